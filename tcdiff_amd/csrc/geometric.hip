// Relational ("geometric") features of generated dances, gfx950: a table of R plane / angle / velocity predicates evaluated at
// every frame of every dancer, each feature the fraction of the frames t = 1 .. T - 1 at which its predicate holds.  float64
// arithmetic on the float32 joints, contraction off (csrc/geo_math.h holds the points and the predicates, and compiles for the
// host too), no atomics; the counts are integers, so the same input gives the same bits.  The definitions:
// include/tcdiff_hip_ext.h.
//
//   geometric_features_kernel   one workgroup of 256 per (clip, dancer): the table staged in LDS once; frames taken 64 at a time
//                               with the frame before them, read in place through their element strides into LDS (a frame's 72
//                               floats at a stride of 73: lane = frame reads touch every bank once), the floor of every staged
//                               frame computed once; wave w takes the rows r = w, w + 4, ..., lane = frame, so a row's kind is
//                               wave-uniform; a (row, chunk)'s count is one ballot, added to an LDS integer only that wave writes
#include "common.h"
#include "geo_math.h"
#include "tcdiff_hip_ext.h"

#define TC_GEO_THREADS 256
#define TC_GEO_WAVES (TC_GEO_THREADS / TC_WAVE)
#define TC_GEO_CHUNK 64                                   // frames per pass = lanes of a wave
#define TC_GEO_LD 73                                      // floats between two staged frames

static_assert(TC_GEO_N_POINTS == TC_GEO_POINTS && TC_GEO_N_KINDS == TC_GEO_FAST + 1, "geo_math.h and the header disagree");

__global__ __launch_bounds__(TC_GEO_THREADS) void geometric_features_kernel(const float* __restrict__ joints, long jsb, long jsd,
                                                                            long jst, int dn, int T, int up,
                                                                            const int* __restrict__ table,
                                                                            const double* __restrict__ range, int R, double tau,
                                                                            double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ float s_fr[(TC_GEO_CHUNK + 1) * TC_GEO_LD];
    __shared__ double s_floor[TC_GEO_CHUNK + 1];
    __shared__ GeoRow s_row[TC_SET_MAX_D];
    __shared__ int s_count[TC_SET_MAX_D];
    const int tid = threadIdx.x, wave = tid / TC_WAVE, lane = tid % TC_WAVE;
    const long q = blockIdx.x;                            // sequence = clip * dn + dancer
    const long c = q / dn;
    const int d = (int)(q - c * dn);
    double* o = out + q * R;
    if (T < 2) {                                          // no frame has a frame before it
        if (tid < R) o[tid] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    if (tid < R) {                                        // R <= TC_SET_MAX_D < the workgroup (the launcher checks)
        GeoRow r;
        r.kind = table[5 * tid];
        r.a = table[5 * tid + 1];
        r.b = table[5 * tid + 2];
        r.c = table[5 * tid + 3];
        r.p = table[5 * tid + 4];
        r.lo = range[2 * tid];
        r.hi = range[2 * tid + 1];
        if (!geo_row_valid(r.kind, r.a, r.b, r.c, r.p)) r.kind = -1;       // counts nothing, reads nothing
        s_row[tid] = r;
        s_count[tid] = 0;
    }
    const float* J = joints + c * jsb + d * jsd;
    for (int t0 = 1; t0 < T; t0 += TC_GEO_CHUNK) {        // frames t0 .. t0 + n - 1; slot s holds frame t0 - 1 + s
        const int n = T - t0 < TC_GEO_CHUNK ? T - t0 : TC_GEO_CHUNK;
        __syncthreads();                                  // the table is staged / the previous chunk has been read
        for (int i = tid; i < (n + 1) * 72; i += TC_GEO_THREADS) {
            const int s = i / 72, e = i - s * 72;
            s_fr[s * TC_GEO_LD + e] = J[(long)(t0 - 1 + s) * jst + e];
        }
        __syncthreads();
        if (tid <= n) s_floor[tid] = geo_floor(s_fr + tid * TC_GEO_LD, up);
        __syncthreads();
        for (int r = wave; r < R; r += TC_GEO_WAVES) {
            const GeoRow row = s_row[r];
            if (row.kind < 0) continue;                   // wave-uniform
            int holds = 0;
            if (lane < n)
                holds = geo_holds(row, s_fr + (lane + 1) * TC_GEO_LD, s_floor[lane + 1], s_fr + lane * TC_GEO_LD, s_floor[lane], up,
                                  tau);
            const unsigned long long m = __ballot(holds);
            if (lane == 0) s_count[r] += __popcll(m);
        }
    }
    __syncthreads();
    if (tid < R) o[tid] = (double)s_count[tid] / (double)(T - 1);
}

extern "C" int tcdiff_geometric_features(const float* joints, const long* joint_strides, int b, int dn, int T, int up,
                                         const int* table, const double* range, int R, double time_per_frame, double* feats,
                                         hipStream_t stream) {
    if (!joints || !joint_strides || !table || !range || !feats) return TC_ERR_ARG;
    if (b < 1 || dn < 1 || T < 1 || R < 1 || up < 0 || up > 2) return TC_ERR_ARG;
    if (!(time_per_frame > 0.0) || !(time_per_frame <= 1.7976931348623157e308)) return TC_ERR_ARG;
    if (R > TC_SET_MAX_D) return TC_ERR_UNSUPPORTED;
    const long Q = (long)b * dn;
    if (Q > 0x7fffffffL) return TC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(geometric_features_kernel, dim3((unsigned)Q), dim3(TC_GEO_THREADS), 0, stream, joints, joint_strides[0],
                       joint_strides[1], joint_strides[2], dn, T, up, table, range, R, time_per_frame, feats);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
