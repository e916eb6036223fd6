// Linear blend skinning of a user-supplied SMPL body, gfx950: exported SMPL poses -> the body's vertices on the device.  The
// definitions, the order of every sum and the error codes: include/tcdiff_skin.h.  No atomics, no workspace beyond the caller's
// feat and A: the same input gives the same bits.
//
//   skin_pose_kernel     one thread per pose (csrc/skin_math.h, float64, contraction off; compiles for the host too): feat [P][208],
//                        A [P][24][12] and, if asked, the posed joints.  The form of pose_export_kernel; not the hot path.
//   skin_vertex_kernel   THE HOT PATH, on v_mfma_f32_32x32x2_f32.  A workgroup of four waves owns TC_SKIN_POSE_TILE = 32 poses x
//                        TC_SKIN_VERT_TILE = 128 vertices, a wave 32 poses x 32 vertices.  The tile's features sit in LDS transposed,
//                        [208][32], so that the A operand of k-pair kp (lane l: pose l & 31, k = 2 kp + (l >> 5)) is the 64
//                        consecutive floats at 64 kp: one conflict-free ds_read_b32.  (Rows of 208 floats, pose-major, would put all 32
//                        poses of a half-wave on 4 banks: 208 = 3 x 64 + 16.)  A and the shifts sit in LDS as they are.  The B
//                        operands are blend[k][3 v + c], c = 0, 1, 2: three dword loads per lane that together cover 96 consecutive
//                        floats per half-wave, each row of blend streamed once per pose tile; three accumulators of 16 floats hold
//                        x, y, z of (pose acc_row(i, l >> 5), vertex l & 31), so the blend, the transform and the shift run on the
//                        accumulators and out is stored once.  The chain of one (pose, vertex, c) is k = 0, 1, .. 207 whatever the
//                        tile, so a vertex's bits do not depend on the tile or batch.  Lanes of poses >= P compute on zeros, lanes of
//                        vertices >= V on vertex V - 1's operands; neither stores.
#include "common.h"
#include "skin_math.h"
#include "tcdiff_skin.h"

#define TC_SKIN_POSE_THREADS 64
#define TC_SKIN_THREADS 256
#define TC_SKIN_KMAX 8

static_assert(TC_SKIN_POSE_TILE == 32, "a pose tile is the M of one v_mfma_f32_32x32x2_f32");
static_assert(TC_SKIN_VERT_TILE == 32 * (TC_SKIN_THREADS / TC_WAVE), "a wave owns 32 vertices");
static_assert(TC_SKIN_FEAT == TC_SKIN_FEAT_USED + 1 && TC_SKIN_FEAT % 2 == 0, "skin_math.h and the header disagree");
static_assert(4 * (TC_SKIN_FEAT * TC_SKIN_POSE_TILE + TC_SKIN_POSE_TILE * 288 + TC_SKIN_POSE_TILE * 4) <= 65536, "LDS");

struct SkinParents { int p[TC_SKIN_JOINTS]; };

__global__ __launch_bounds__(TC_SKIN_POSE_THREADS) void skin_pose_kernel(const float* __restrict__ poses, const float* __restrict__ trans,
                                                                        int P, const float* __restrict__ J,
                                                                        const float* __restrict__ offsets, SkinParents parents,
                                                                        int smpl_origin, float* __restrict__ feat,
                                                                        float* __restrict__ A, float* __restrict__ joints_out) {
    const long p = (long)blockIdx.x * TC_SKIN_POSE_THREADS + threadIdx.x;
    if (p >= P) return;
    double G[TC_SKIN_JOINTS * 12];
    skin_pose(poses + p * 72, trans + p * 3, J, offsets, parents.p, smpl_origin, G, feat + p * TC_SKIN_FEAT, A + p * 288,
              joints_out ? joints_out + p * 72 : nullptr);
}

template <int K>
__global__ __launch_bounds__(TC_SKIN_THREADS) void skin_vertex_kernel(const float* __restrict__ feat, const float* __restrict__ A,
                                                                     const float* __restrict__ trans, const float* __restrict__ J,
                                                                     const float* __restrict__ v_shaped, const float* __restrict__ blend,
                                                                     const float* __restrict__ weights, const int* __restrict__ wj,
                                                                     int P, int V, int pose_blend, int smpl_origin,
                                                                     float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_feat[TC_SKIN_FEAT * TC_SKIN_POSE_TILE];      // [k][pose]
    __shared__ __attribute__((aligned(16))) float s_A[TC_SKIN_POSE_TILE * 288];                  // [pose][joint][12]
    __shared__ float s_shift[TC_SKIN_POSE_TILE * 4];                                             // [pose][3], padded to 4
    const int tid = threadIdx.x, lane = tid % TC_WAVE, wave = tid / TC_WAVE;
    const int nvt = (V + TC_SKIN_VERT_TILE - 1) / TC_SKIN_VERT_TILE;                             // vertex tiles fastest: a 1-D grid
    const int pt = blockIdx.x / nvt, vt = blockIdx.x - pt * nvt;
    const int p0 = pt * TC_SKIN_POSE_TILE;
    const int np = min(TC_SKIN_POSE_TILE, P - p0);                                               // >= 1

    // the tile's features (transposed) and transforms; poses past P are zeros
    for (int i = tid; i < TC_SKIN_POSE_TILE * (TC_SKIN_FEAT / 4); i += TC_SKIN_THREADS) {
        const int m = i / (TC_SKIN_FEAT / 4), k4 = i - m * (TC_SKIN_FEAT / 4);
        f32x4_t v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (m < np) v = *reinterpret_cast<const f32x4_t*>(feat + (long)(p0 + m) * TC_SKIN_FEAT + 4 * k4);
#pragma unroll
        for (int e = 0; e < 4; ++e) s_feat[(4 * k4 + e) * TC_SKIN_POSE_TILE + m] = v[e];
    }
    for (int i = tid; i < TC_SKIN_POSE_TILE * 72; i += TC_SKIN_THREADS) {
        const int m = i / 72;
        f32x4_t v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (m < np) v = *reinterpret_cast<const f32x4_t*>(A + (long)p0 * 288 + 4L * i);
        *reinterpret_cast<f32x4_t*>(s_A + 4 * i) = v;
    }
    if (tid < TC_SKIN_POSE_TILE * 3) {
        const int m = tid / 3, c = tid - 3 * m;
        s_shift[4 * m + c] = m < np ? skin_shift(trans[(long)(p0 + m) * 3 + c], J[c], smpl_origin) : 0.0f;
    }
    __syncthreads();

    const int col = lane & 31, half = lane >> 5;
    const int v = vt * TC_SKIN_VERT_TILE + wave * 32 + col;
    const int vc = min(v, V - 1);                                                                // the operands' vertex: in range
    f32x16_t ax = {0}, ay = {0}, az = {0};
    if (pose_blend) {
        const long ld = 3L * V;
        const float* b = blend + 3L * vc + (long)half * ld;                                      // row k = 2 kp + half
        const float* a = s_feat + lane;
#pragma unroll 4
        for (int kp = 0; kp < TC_SKIN_FEAT / 2 - 1; ++kp) {                                      // (hipcc unrolls it whole: the loads run ahead)
            const float fa = a[kp * 64];
            const float bx = b[0], by = b[1], bz = b[2];
            b += 2 * ld;
            ax = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, bx, ax, 0, 0, 0);
            ay = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, by, ay, 0, 0, 0);
            az = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, bz, az, 0, 0, 0);
        }
        {                                                                                        // k = 206 and the zero row 207
            const float fa = a[(TC_SKIN_FEAT / 2 - 1) * 64];
            float bx = 0.0f, by = 0.0f, bz = 0.0f;
            if (half == 0) { bx = b[0]; by = b[1]; bz = b[2]; }
            ax = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, bx, ax, 0, 0, 0);
            ay = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, by, ay, 0, 0, 0);
            az = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, bz, az, 0, 0, 0);
        }
    }

    const float sx = v_shaped[3L * vc], sy = v_shaped[3L * vc + 1], sz = v_shaped[3L * vc + 2];
    float w[K];
    int jo[K];                                                                                   // the joint's offset into a pose's A
#pragma unroll
    for (int s = 0; s < K; ++s) {
        w[s] = weights[(long)vc * K + s];
        jo[s] = wj[(long)vc * K + s] * 12;
    }
    if (v >= V) return;                                                                          // no barrier follows
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int m = acc_row(i, half);
        if (m >= np) continue;
        const float x = sx + ax[i], y = sy + ay[i], z = sz + az[i];
        f32x4_t t0 = {0.0f, 0.0f, 0.0f, 0.0f}, t1 = t0, t2 = t0;
#pragma unroll
        for (int s = 0; s < K; ++s) {
            const f32x4_t* q = reinterpret_cast<const f32x4_t*>(s_A + m * 288 + jo[s]);
            const f32x4_t q0 = q[0], q1 = q[1], q2 = q[2];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                t0[e] = fmaf(w[s], q0[e], t0[e]);
                t1[e] = fmaf(w[s], q1[e], t1[e]);
                t2[e] = fmaf(w[s], q2[e], t2[e]);
            }
        }
        float* o = out + ((long)(p0 + m) * V + v) * 3;
        o[0] = (fmaf(t0[2], z, fmaf(t0[1], y, fmaf(t0[0], x, 0.0f))) + t0[3]) + s_shift[4 * m];
        o[1] = (fmaf(t1[2], z, fmaf(t1[1], y, fmaf(t1[0], x, 0.0f))) + t1[3]) + s_shift[4 * m + 1];
        o[2] = (fmaf(t2[2], z, fmaf(t2[1], y, fmaf(t2[0], x, 0.0f))) + t2[3]) + s_shift[4 * m + 2];
    }
}

template <int K>
static void skin_launch_vertices(dim3 grid, hipStream_t stream, const float* feat, const float* A, const float* trans, const float* J,
                                 const float* v_shaped, const float* blend, const float* weights, const int* wj, int P, int V,
                                 int pose_blend, int smpl_origin, float* out) {
    hipLaunchKernelGGL(skin_vertex_kernel<K>, grid, dim3(TC_SKIN_THREADS), 0, stream, feat, A, trans, J, v_shaped, blend, weights, wj, P,
                       V, pose_blend, smpl_origin, out);
}

extern "C" int tcs_skin_vertices(const float* smpl_poses, const float* smpl_trans, int P, const float* v_shaped, const float* blend,
                                 const float* joints, const float* offsets, const int* parents, const float* weights,
                                 const int* weight_joints, int V, int K, int pose_blend, int origin, float* feat, float* A,
                                 float* joints_out, float* out, hipStream_t stream) {
    if (!smpl_poses || !smpl_trans || !v_shaped || !blend || !joints || !offsets || !parents || !weights || !weight_joints || !feat ||
        !A || !out)
        return TC_ERR_ARG;
    if (P < 1 || V < 1 || K < 1 || K > TC_SKIN_KMAX) return TC_ERR_ARG;
    if (pose_blend < 0 || pose_blend > 1) return TC_ERR_ARG;
    if (origin != TC_SKIN_ORIGIN_PELVIS && origin != TC_SKIN_ORIGIN_SMPL) return TC_ERR_ARG;
    SkinParents par;
    int roots = 0;
    for (int j = 0; j < TC_SKIN_JOINTS; ++j) {
        par.p[j] = parents[j];
        if (parents[j] < 0 || parents[j] >= TC_SKIN_JOINTS) ++roots;
        else if (parents[j] >= j) return TC_ERR_ARG;
    }
    if (roots != 1) return TC_ERR_ARG;                                   // with every parent before its child, the root is joint 0
    if ((reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(A)) & 15) return TC_ERR_ALIGN;
    const long lim = 0x7fffffffL;
    if ((long)P * V > lim / 3 || (long)P > lim / 288) return TC_ERR_UNSUPPORTED;
    const int smpl_origin = origin == TC_SKIN_ORIGIN_SMPL;
    hipLaunchKernelGGL(skin_pose_kernel, dim3((unsigned)((P + TC_SKIN_POSE_THREADS - 1) / TC_SKIN_POSE_THREADS)),
                       dim3(TC_SKIN_POSE_THREADS), 0, stream, smpl_poses, smpl_trans, P, joints, offsets, par, smpl_origin, feat, A,
                       joints_out);
    TC_CHECK_LAUNCH();
    const long tiles = (long)((V + TC_SKIN_VERT_TILE - 1) / TC_SKIN_VERT_TILE) * ((P + TC_SKIN_POSE_TILE - 1) / TC_SKIN_POSE_TILE);
    const dim3 grid((unsigned)tiles);                                    // tiles <= P V < 2^31 / 3
    switch (K) {
#define TC_SKIN_CASE(k)                                                                                                              \
    case k:                                                                                                                          \
        skin_launch_vertices<k>(grid, stream, feat, A, smpl_trans, joints, v_shaped, blend, weights, weight_joints, P, V, pose_blend, \
                                smpl_origin, out);                                                                                   \
        break;
        TC_SKIN_CASE(1) TC_SKIN_CASE(2) TC_SKIN_CASE(3) TC_SKIN_CASE(4) TC_SKIN_CASE(5) TC_SKIN_CASE(6) TC_SKIN_CASE(7) TC_SKIN_CASE(8)
#undef TC_SKIN_CASE
    }
    TC_CHECK_LAUNCH();
    return TC_OK;
}
