// Mesh-level contact between the dancers' skinned bodies (include/tcdiff_meshcontact.h), gfx950.  Three launches for any number of clips:
//   1. boxes:   one workgroup per pose -- the float32 box of its V vertices and the finite flag, wave shuffles and one LDS round
//   2. contact: one workgroup per (clip, frame, ordered pair a -> b); it leaves at once when the frame is invalid or the boxes rule
//               contact out.  Otherwise a's vertices in chunks of 256, those inside b's box (floor plane, and not above it) compacted
//               by ballot and prefix into an LDS list of at most TC_MESH_CANDIDATES; b's faces in chunks of 256, those whose
//               floor-plane box meets the candidates' and that reach the lowest candidate compacted the same way into an LDS tile
//               of at most TC_MESH_TILE faces (nine floats and the order flags); candidates x tile, a lane per candidate, every lane
//               reading the same face (an LDS broadcast) and testing its floor-plane box first, the winding counts in registers; the
//               inside candidates compacted in place;
//               for those alone the distance pass over ALL faces, tile by tile, a wave per vertex, the lanes over the faces (stride
//               nine words: conflict-free), a face skipped when its box is further from the vertex than the nearest face above it
//               (float32 with slack, meshcontact_math.h: it never skips the nearest face), a cross-lane minimum of the squared
//               distances, one root, and the arg-max over the total order.
//   3. reduce:  one workgroup per (clip, pair) -- the frames for the rate, the episodes, the mean and the arg-max; the frame planes.
// No atomics; counts are integers, every minimum is of numbers (exact, order-free), every maximum is over a total order: the same
// input gives the same bits.  The arithmetic is csrc/meshcontact_math.h (shared with the host build of tests/host).  LDS per
// workgroup of launch 2: 16 KiB of candidates, 20 KiB of tile, 12 KiB of depths and bounds -- three workgroups a CU and room to spare.
#include "common.h"
#include "meshcontact_math.h"
#include "tcdiff_meshcontact.h"

#define TCM_THREADS TC_MESH_THREADS
#define TCM_WAVES (TCM_THREADS / 64)
#define TCM_ROUNDS (TC_MESH_CANDIDATES / TCM_THREADS)
static_assert(TC_MESH_LAUNCHES == 3, "three launches");
static_assert(TCM_THREADS == 256 && TC_MESH_CANDIDATES % TCM_THREADS == 0 && TC_MESH_TILE % TCM_THREADS == 0, "chunks of one workgroup");
static_assert(TC_MESH_WS_POSE == 8 * 4 && TC_MESH_WS_ORDERED == 8 + 4 + 4, "the header states the workspace");

struct TcmOrdered { double depth; int count; int vertex; };          // what launch 2 leaves per (clip, frame, pair, direction)
static_assert(sizeof(TcmOrdered) == TC_MESH_WS_ORDERED, "sixteen bytes");

// pair p of dn dancers in lexicographic order -> (a, b), a < b
DEVINL void tcm_pair_of(int p, int dn, int* a, int* b) {
    int first = 0;
    while (p >= dn - 1 - first) {
        p -= dn - 1 - first;
        ++first;
    }
    *a = first;
    *b = first + 1 + p;
}

// ---- launch 1 -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TCM_THREADS) void mesh_boxes_kernel(const float* __restrict__ vertices, long s0, long s1, int rows, int V,
                                                                  float* __restrict__ box) {
    __shared__ float s_lo[TCM_WAVES][3], s_hi[TCM_WAVES][3];
    __shared__ int s_ok[TCM_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long pose = blockIdx.x;                             // clip rows + row, row = frame dn + dancer
    const long c = pose / rows;
    const float* X = vertices + c * s0 + (pose - c * rows) * s1;
    const float inf = __int_as_float(0x7f800000);
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    int ok = 1;
    for (int v = tid; v < V; v += TCM_THREADS) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float x = X[3 * (long)v + k];
            ok &= tcm_finite32(x);
            lo[k] = x < lo[k] ? x : lo[k];
            hi[k] = x > hi[k] ? x : hi[k];
        }
    }
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float l = __shfl_xor(lo[k], o), h = __shfl_xor(hi[k], o);
            lo[k] = l < lo[k] ? l : lo[k];
            hi[k] = h > hi[k] ? h : hi[k];
        }
        ok &= __shfl_xor(ok, o);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s_lo[wave][k] = lo[k];
            s_hi[wave][k] = hi[k];
        }
        s_ok[wave] = ok;
    }
    __syncthreads();
    if (tid < 3) {
        float l = s_lo[0][tid], h = s_hi[0][tid];
        for (int w = 1; w < TCM_WAVES; ++w) {
            l = s_lo[w][tid] < l ? s_lo[w][tid] : l;
            h = s_hi[w][tid] > h ? s_hi[w][tid] : h;
        }
        box[8 * pose + tid] = l;
        box[8 * pose + 3 + tid] = h;
    }
    if (tid == 3) {
        int all = 1;
        for (int w = 0; w < TCM_WAVES; ++w) all &= s_ok[w];
        box[8 * pose + 6] = all ? 1.0f : 0.0f;
        box[8 * pose + 7] = 0.0f;
    }
}

// ---- launch 2 -------------------------------------------------------------------------------------------------------------------------------
// where a thread with `keep` writes in a compacted list, and how many of the workgroup keep: ballot and prefix in the wave, the four
// wave totals through LDS.  Two barriers; every thread of the workgroup calls it.
DEVINL int tcm_compact(bool keep, int* s_wave, int* total) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned long long mask = __ballot(keep);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    __syncthreads();                                          // the previous totals have been read
    if (lane == 0) s_wave[wave] = __popcll(mask);
    __syncthreads();
    int base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < TCM_WAVES; ++w) {
        const int n = s_wave[w];
        base += w < wave ? n : 0;
        all += n;
    }
    *total = all;
    return base + before;
}

// face f of the body X -> nine floats (x, y, z of A, B, C in the header's sense) and its order flags
DEVINL int tcm_load_face(const int* __restrict__ faces, const float* __restrict__ X, int f, int ax, int ay, int az, float* v) {
    const int i0 = faces[3 * (long)f], i1 = faces[3 * (long)f + 1], i2 = faces[3 * (long)f + 2];
    const float* A = X + 3 * (long)i0;
    const float* B = X + 3 * (long)i1;
    const float* C = X + 3 * (long)i2;
    v[0] = A[ax]; v[1] = A[ay]; v[2] = A[az];
    v[3] = B[ax]; v[4] = B[ay]; v[5] = B[az];
    v[6] = C[ax]; v[7] = C[ay]; v[8] = C[az];
    return tcm_flags(i0, i1, i2);
}

DEVINL float tcm_min3(float a, float b, float c) { const float m = a < b ? a : b; return m < c ? m : c; }
DEVINL float tcm_max3(float a, float b, float c) { const float m = a > b ? a : b; return m > c ? m : c; }

__global__ __launch_bounds__(TCM_THREADS) void mesh_contact_kernel(const float* __restrict__ vertices, long s0, long s1,
                                                                    const int* __restrict__ faces, int dn, int T, int V, int F, int P, int up,
                                                                    const float* __restrict__ box, TcmOrdered* __restrict__ out) {
    __shared__ float s_cand[TC_MESH_CANDIDATES * 3];
    __shared__ int s_idx[TC_MESH_CANDIDATES];
    __shared__ float s_tile[TC_MESH_TILE * 9];
    __shared__ int s_flag[TC_MESH_TILE];
    __shared__ double s_depth[TC_MESH_CANDIDATES];
    __shared__ float s_ub[TC_MESH_CANDIDATES];
    __shared__ int s_wave[TCM_WAVES];
    __shared__ float s_box[TCM_WAVES][5];
    __shared__ double s_bd[TCM_WAVES];
    __shared__ int s_bv[TCM_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long item = blockIdx.x;                             // ((clip T + frame) P + pair) 2 + direction
    const int dir = (int)(item & 1);
    const long ctp = item >> 1;
    const long ct = ctp / P;                                  // clip T + frame
    int a, b;
    tcm_pair_of((int)(ctp - ct * P), dn, &a, &b);
    const int src = dir ? b : a, dst = dir ? a : b;           // src's vertices, inside dst's body?
    const long c = ct / T;
    const long t = ct - c * T;
    const long rows = (long)T * dn;
    const float* bs = box + 8 * (c * rows + t * dn + src);
    const float* bd = box + 8 * (c * rows + t * dn + dst);
    const int ax = tcm_axis_x(up), ay = tcm_axis_y(up), az = up;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (bs[6] == 0.0f || bd[6] == 0.0f) {                     // an invalid frame
        if (tid == 0) {
            TcmOrdered r;
            r.depth = nan; r.count = -1; r.vertex = -1;
            out[item] = r;
        }
        return;
    }
    const float dlo_x = bd[ax], dhi_x = bd[3 + ax], dlo_y = bd[ay], dhi_y = bd[3 + ay], dhi_z = bd[3 + az];
    if (bs[ax] > dhi_x || bs[3 + ax] < dlo_x || bs[ay] > dhi_y || bs[3 + ay] < dlo_y || bs[az] > dhi_z) {
        if (tid == 0) {
            TcmOrdered r;
            r.depth = 0.0; r.count = 0; r.vertex = -1;
            out[item] = r;
        }
        return;
    }
    const float* Xs = vertices + c * s0 + (t * dn + src) * s1;
    const float* Xd = vertices + c * s0 + (t * dn + dst) * s1;
    const float inf = __int_as_float(0x7f800000);
    const double dinf = __longlong_as_double(0x7ff0000000000000LL);
    int count = 0, best_v = -1;                               // uniform over the workgroup
    double best_d = 0.0;

    for (int v0 = 0; v0 < V;) {
        // ---- the candidates: src's vertices that pass the box test, until the list could overflow ----
        int n = 0;
        while (v0 < V && n <= TC_MESH_CANDIDATES - TCM_THREADS) {
            const int v = v0 + tid;
            float px = 0.0f, py = 0.0f, pz = 0.0f;
            bool keep = false;
            if (v < V) {
                px = Xs[3 * (long)v + ax];
                py = Xs[3 * (long)v + ay];
                pz = Xs[3 * (long)v + az];
                keep = px >= dlo_x && px <= dhi_x && py >= dlo_y && py <= dhi_y && pz <= dhi_z;
            }
            int total;
            const int at = n + tcm_compact(keep, s_wave, &total);
            if (keep) {
                s_cand[3 * at] = px;
                s_cand[3 * at + 1] = py;
                s_cand[3 * at + 2] = pz;
                s_idx[at] = v;
            }
            n += total;
            v0 += TCM_THREADS;
        }
        __syncthreads();                                      // the list is complete
        if (n == 0) continue;
        // ---- the candidates' floor-plane box and their lowest point ----
        float cl_x = inf, ch_x = -inf, cl_y = inf, ch_y = -inf, cl_z = inf;
        for (int i = tid; i < n; i += TCM_THREADS) {
            const float x = s_cand[3 * i], y = s_cand[3 * i + 1], z = s_cand[3 * i + 2];
            cl_x = x < cl_x ? x : cl_x; ch_x = x > ch_x ? x : ch_x;
            cl_y = y < cl_y ? y : cl_y; ch_y = y > ch_y ? y : ch_y;
            cl_z = z < cl_z ? z : cl_z;
        }
        for (int o = 32; o >= 1; o >>= 1) {
            float q;
            q = __shfl_xor(cl_x, o); cl_x = q < cl_x ? q : cl_x;
            q = __shfl_xor(ch_x, o); ch_x = q > ch_x ? q : ch_x;
            q = __shfl_xor(cl_y, o); cl_y = q < cl_y ? q : cl_y;
            q = __shfl_xor(ch_y, o); ch_y = q > ch_y ? q : ch_y;
            q = __shfl_xor(cl_z, o); cl_z = q < cl_z ? q : cl_z;
        }
        if (lane == 0) {
            s_box[wave][0] = cl_x; s_box[wave][1] = ch_x; s_box[wave][2] = cl_y; s_box[wave][3] = ch_y; s_box[wave][4] = cl_z;
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < TCM_WAVES; ++w) {
            cl_x = s_box[w][0] < cl_x ? s_box[w][0] : cl_x; ch_x = s_box[w][1] > ch_x ? s_box[w][1] : ch_x;
            cl_y = s_box[w][2] < cl_y ? s_box[w][2] : cl_y; ch_y = s_box[w][3] > ch_y ? s_box[w][3] : ch_y;
            cl_z = s_box[w][4] < cl_z ? s_box[w][4] : cl_z;
        }
        // ---- the winding counts: candidates x the faces that can cover one of them ----
        float p[TCM_ROUNDS][3];
        double above[TCM_ROUNDS];                             // the nearest counted face above the candidate: its depth is at most that
        int w[TCM_ROUNDS];
#pragma unroll
        for (int k = 0; k < TCM_ROUNDS; ++k) {
            const int i = tid + k * TCM_THREADS;
            w[k] = 0;
            above[k] = dinf;
#pragma unroll
            for (int e = 0; e < 3; ++e) p[k][e] = i < n ? s_cand[3 * i + e] : 0.0f;
        }
        for (int f0 = 0; f0 < F;) {
            int m = 0;
            while (f0 < F && m <= TC_MESH_TILE - TCM_THREADS) {
                const int f = f0 + tid;
                float fv[9];
                int flags = 0;
                bool keep = false;
                if (f < F) {
                    flags = tcm_load_face(faces, Xd, f, ax, ay, az, fv);
                    keep = tcm_max3(fv[0], fv[3], fv[6]) >= cl_x && tcm_min3(fv[0], fv[3], fv[6]) <= ch_x &&
                           tcm_max3(fv[1], fv[4], fv[7]) >= cl_y && tcm_min3(fv[1], fv[4], fv[7]) <= ch_y &&
                           tcm_max3(fv[2], fv[5], fv[8]) >= cl_z;
                }
                int total;
                const int at = m + tcm_compact(keep, s_wave, &total);
                if (keep) {
#pragma unroll
                    for (int e = 0; e < 9; ++e) s_tile[9 * at + e] = fv[e];
                    s_flag[at] = flags;
                }
                m += total;
                f0 += TCM_THREADS;
            }
            __syncthreads();                                  // the tile is complete
            for (int j = 0; j < m; ++j) {
                float ff[9];
#pragma unroll
                for (int e = 0; e < 9; ++e) ff[e] = s_tile[9 * j + e];
                const int flags = s_flag[j];
                // a face covers p only if p lies in its floor-plane box (the header's broad phase: exact float32 compares)
                const float lx = tcm_min3(ff[0], ff[3], ff[6]), hx = tcm_max3(ff[0], ff[3], ff[6]);
                const float ly = tcm_min3(ff[1], ff[4], ff[7]), hy = tcm_max3(ff[1], ff[4], ff[7]);
#pragma unroll
                for (int k = 0; k < TCM_ROUNDS; ++k)
                    if (tid + k * TCM_THREADS < n && p[k][0] >= lx && p[k][0] <= hx && p[k][1] >= ly && p[k][1] <= hy) {
                        double fa[9], gap, area;
#pragma unroll
                        for (int e = 0; e < 9; ++e) fa[e] = (double)ff[e];
                        const double q[3] = {(double)p[k][0], (double)p[k][1], (double)p[k][2]};
                        const int sign = tcm_wind_gap(q, fa, fa + 3, fa + 6, flags, &gap, &area);
                        if (sign != 0) {
                            w[k] += sign;
                            if ((area >= TCM_MIN_AREA || area <= -TCM_MIN_AREA) && gap < above[k]) above[k] = gap;
                        }
                    }
            }
            __syncthreads();                                  // the tile has been read
        }
        // ---- the inside candidates, compacted in place (a round writes below what later rounds read) ----
        int ni = 0;
#pragma unroll
        for (int k = 0; k < TCM_ROUNDS; ++k) {
            const int i = tid + k * TCM_THREADS;
            const bool keep = i < n && w[k] != 0;
            const int idx = i < n ? s_idx[i] : 0;
            const float x = i < n ? s_cand[3 * i] : 0.0f, y = i < n ? s_cand[3 * i + 1] : 0.0f, z = i < n ? s_cand[3 * i + 2] : 0.0f;
            int total;
            const int at = ni + tcm_compact(keep, s_wave, &total);          // its barriers stand between the reads above and the writes
            if (keep) {
                s_cand[3 * at] = x;
                s_cand[3 * at + 1] = y;
                s_cand[3 * at + 2] = z;
                s_idx[at] = idx;
                s_ub[at] = tcm_bound2((float)above[k]);       // +inf where no face gave a bound: nothing is skipped
            }
            ni += total;
        }
        count += ni;
        if (ni == 0) {
            __syncthreads();                                  // the list has been read before the next batch overwrites it
            continue;
        }
        // ---- the depth of the inside vertices: every face, a wave per vertex ----
        for (int j = tid; j < ni; j += TCM_THREADS) s_depth[j] = dinf;
        for (int f0 = 0; f0 < F; f0 += TC_MESH_TILE) {
            const int m = F - f0 < TC_MESH_TILE ? F - f0 : TC_MESH_TILE;
            __syncthreads();                                  // the previous tile has been read; s_cand and s_depth are written
            for (int j = tid; j < m; j += TCM_THREADS) {
                float fv[9];
                tcm_load_face(faces, Xd, f0 + j, ax, ay, az, fv);
#pragma unroll
                for (int e = 0; e < 9; ++e) s_tile[9 * j + e] = fv[e];
            }
            __syncthreads();
            for (int j = wave; j < ni; j += TCM_WAVES) {
                const float qf[3] = {s_cand[3 * j], s_cand[3 * j + 1], s_cand[3 * j + 2]};
                const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
                float bound = s_ub[j];                        // squared; it only ever falls
                double dmin = dinf;                           // the smallest SQUARED distance of this lane's faces
                for (int l = lane; l < m; l += 64) {
                    float ff[9];
#pragma unroll
                    for (int e = 0; e < 9; ++e) ff[e] = s_tile[9 * l + e];
                    if (tcm_box_dist2(qf, ff) > bound) continue;          // the face's box is further than the depth can be
                    double fa[9];
#pragma unroll
                    for (int e = 0; e < 9; ++e) fa[e] = (double)ff[e];
                    const double d = tcm_tri_dist2(q, fa, fa + 3, fa + 6);
                    if (d < dmin) {                           // a NaN takes no part
                        dmin = d;
                        bound = tcm_fmin(bound, (float)d * 1.01f + 1e-9f);
                    }
                }
                for (int o = 32; o >= 1; o >>= 1) {
                    const double other = __shfl_xor(dmin, o);
                    dmin = other < dmin ? other : dmin;
                }
                if (lane == 0 && dmin < s_depth[j]) s_depth[j] = dmin;          // vertex j belongs to this wave alone
            }
        }
        __syncthreads();                                      // every squared depth is final
        for (int j = tid; j < ni; j += TCM_THREADS) s_depth[j] = sqrt(s_depth[j]);          // monotone: the root of the minimum
        __syncthreads();
        // ---- the deepest of them: the larger depth, then the lower vertex ----
        double md = 0.0;
        int mv = -1;
        for (int j = tid; j < ni; j += TCM_THREADS)
            if (tcm_deeper(s_depth[j], s_idx[j], md, mv)) {
                md = s_depth[j];
                mv = s_idx[j];
            }
        for (int o = 32; o >= 1; o >>= 1) {
            const double od = __shfl_xor(md, o);
            const int ov = __shfl_xor(mv, o);
            if (tcm_deeper(od, ov, md, mv)) {
                md = od;
                mv = ov;
            }
        }
        if (lane == 0) {
            s_bd[wave] = md;
            s_bv[wave] = mv;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < TCM_WAVES; ++k)
            if (tcm_deeper(s_bd[k], s_bv[k], best_d, best_v)) {
                best_d = s_bd[k];
                best_v = s_bv[k];
            }
        __syncthreads();                                      // the lists and the wave results have been read
    }
    if (tid == 0) {
        TcmOrdered r;
        r.depth = best_d; r.count = count; r.vertex = best_v;
        out[item] = r;
    }
}

// ---- launch 3 -------------------------------------------------------------------------------------------------------------------------------
DEVINL long tcm_block_sum(long x, long* red) {
    const int tid = threadIdx.x;
    __syncthreads();                                          // the previous total has been read
    red[tid] = x;
    __syncthreads();
    for (int o = TCM_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = red[tid] + red[tid + o];
        __syncthreads();
    }
    return red[0];
}

DEVINL bool tcm_contact_at(const TcmOrdered* __restrict__ o, long t, int P) {
    const TcmOrdered* f = o + t * P * 2;
    return f[0].count >= 0 && f[0].count + f[1].count > 0;
}

__global__ __launch_bounds__(TCM_THREADS) void mesh_reduce_kernel(const TcmOrdered* __restrict__ ordered, int dn, int T, int V, int P,
                                                                   int* __restrict__ inside, double* __restrict__ depth,
                                                                   double* __restrict__ rate, long* __restrict__ episodes,
                                                                   double* __restrict__ depth_max, long* __restrict__ deepest,
                                                                   double* __restrict__ inside_mean) {
#pragma clang fp contract(off)
    __shared__ long s_cnt[TCM_THREADS];
    __shared__ double s_val[TCM_THREADS];
    __shared__ long s_key[TCM_THREADS];
    const int tid = threadIdx.x;
    const long cp = blockIdx.x;                               // clip P + pair
    const long c = cp / P;
    const int p = (int)(cp - c * P);
    int a, b;
    tcm_pair_of(p, dn, &a, &b);
    const TcmOrdered* o = ordered + (c * T * P + p) * 2;      // frame t of this pair: o + t P 2, both directions side by side
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    long n_valid = 0, n_contact = 0, n_start = 0, n_inside = 0, bk = -1;
    double bdep = 0.0;
    for (int t = tid; t < T; t += TCM_THREADS) {
        const TcmOrdered f0 = o[(long)t * P * 2], f1 = o[(long)t * P * 2 + 1];
        const bool valid = f0.count >= 0;
        const bool contact = valid && f0.count + f1.count > 0;
        double d = valid ? 0.0 : nan;
        if (contact) {
            const int second = f0.count == 0 || (f1.count > 0 && f1.depth > f0.depth);          // a tie goes to the lower dancer
            d = second ? f1.depth : f0.depth;
            const long key = ((long)t * 2 + second) * V + (second ? f1.vertex : f0.vertex);
            if (tcm_deeper(d, key, bdep, bk)) {
                bdep = d;
                bk = key;
            }
        }
        n_valid += valid;
        n_contact += contact;
        n_start += contact && !(t > 0 && tcm_contact_at(o, t - 1, P));          // a run starts here
        n_inside += valid ? (long)f0.count + f1.count : 0;
        if (inside) {
            inside[(cp * T + t) * 2] = f0.count;
            inside[(cp * T + t) * 2 + 1] = f1.count;
        }
        if (depth) depth[cp * T + t] = d;
    }
    n_valid = tcm_block_sum(n_valid, s_cnt);
    n_contact = tcm_block_sum(n_contact, s_cnt);
    n_start = tcm_block_sum(n_start, s_cnt);
    n_inside = tcm_block_sum(n_inside, s_cnt);
    s_val[tid] = bdep;
    s_key[tid] = bk;
    __syncthreads();
    for (int w = TCM_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w && tcm_deeper(s_val[tid + w], s_key[tid + w], s_val[tid], s_key[tid])) {
            s_val[tid] = s_val[tid + w];
            s_key[tid] = s_key[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const long key = s_key[0];
        rate[cp] = n_valid ? (double)n_contact / (double)n_valid : nan;
        episodes[cp] = n_start;
        inside_mean[cp] = n_valid ? (double)n_inside / (double)n_valid : nan;
        depth_max[cp] = key < 0 ? 0.0 : s_val[0];
        const long tv = key < 0 ? 0 : key / V;                // frame 2 + direction
        deepest[3 * cp] = key < 0 ? -1 : tv / 2;
        deepest[3 * cp + 1] = key < 0 ? -1 : (tv & 1 ? b : a);
        deepest[3 * cp + 2] = key < 0 ? -1 : key - tv * V;
    }
}

// ---- the entry points ---------------------------------------------------------------------------------------------------------------------
struct TcmShape { long P, poses, ordered; };

static int tcm_shape(int b, int dn, int T, int V, int F, TcmShape* s) {
    if (b < 1 || dn < 1 || T < 1 || V < 1 || F < 1) return TC_ERR_ARG;
    const long lim = 0x7fffffffl;
    s->P = (long)dn * (dn - 1) / 2;
    if ((long)b > lim / T || (long)b * T > lim / dn) return TC_ERR_UNSUPPORTED;
    s->poses = (long)b * T * dn;
    if (s->poses > lim / 3 / V || F > lim / 3) return TC_ERR_UNSUPPORTED;
    if (s->P > 0 && (long)b * T > lim / 2 / s->P) return TC_ERR_UNSUPPORTED;
    s->ordered = (long)b * T * s->P * 2;
    return TC_OK;
}

static long tcm_bytes(const TcmShape& s) { return s.poses * TC_MESH_WS_POSE + s.ordered * TC_MESH_WS_ORDERED; }

extern "C" int tcm_mesh_contact_workspace(int b, int dn, int T, int V, int F, long* bytes) {
    if (!bytes) return TC_ERR_ARG;
    TcmShape s;
    const int rc = tcm_shape(b, dn, T, V, F, &s);
    if (rc != TC_OK) return rc;
    *bytes = tcm_bytes(s);
    return TC_OK;
}

extern "C" int tcm_mesh_contact(const float* vertices, const long* vertex_strides, const int* faces, const int* faces_host, int b, int dn,
                                int T, int V, int F, int up, void* workspace, long workspace_bytes, int* inside, double* depth,
                                double* rate, long* episodes, double* depth_max, long* deepest, double* inside_mean,
                                hipStream_t stream) {
    if (!vertices || !vertex_strides || !faces || !faces_host || !workspace || !rate || !episodes || !depth_max || !deepest || !inside_mean)
        return TC_ERR_ARG;
    if (b < 1 || dn < 1 || T < 1 || V < 1 || F < 1 || up < 0 || up > 2) return TC_ERR_ARG;
    TcmShape s;
    const int rc = tcm_shape(b, dn, T, V, F, &s);
    if (rc != TC_OK) return rc;
    if (vertex_strides[0] < 0 || vertex_strides[1] < 0) return TC_ERR_ARG;
    for (long k = 0; k < 3 * (long)F; ++k)
        if (faces_host[k] < 0 || faces_host[k] >= V) return TC_ERR_ARG;
    if (workspace_bytes < tcm_bytes(s)) return TC_ERR_ARG;
    if ((uintptr_t)workspace % 8 || (uintptr_t)depth % 8 || (uintptr_t)inside % 4) return TC_ERR_ALIGN;
    if (s.P == 0) return TC_OK;                               // one dancer: no pair, nothing to launch
    // the workspace: the ordered results [b T P 2] (sixteen bytes each), then the boxes [b T dn][8] floats
    TcmOrdered* ordered = (TcmOrdered*)workspace;
    float* box = (float*)(ordered + s.ordered);
    const long s0 = vertex_strides[0], s1 = vertex_strides[1];
    const int P = (int)s.P;
    hipLaunchKernelGGL(mesh_boxes_kernel, dim3((unsigned)s.poses), dim3(TCM_THREADS), 0, stream, vertices, s0, s1, T * dn, V, box);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(mesh_contact_kernel, dim3((unsigned)s.ordered), dim3(TCM_THREADS), 0, stream, vertices, s0, s1, faces, dn, T, V, F, P,
                       up, (const float*)box, ordered);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(mesh_reduce_kernel, dim3((unsigned)((long)b * P)), dim3(TCM_THREADS), 0, stream, (const TcmOrdered*)ordered, dn, T, V,
                       P, inside, depth, rate, episodes, depth_max, deepest, inside_mean);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
