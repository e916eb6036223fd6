// Set-level metrics of generated dances, gfx950: Bailando's kinetic features of the joint positions csrc/export.hip leaves on the
// device, and FID / diversity of a set of feature rows against a reference set.  float64 arithmetic throughout, contraction off in
// the whole file, no atomics, no host synchronisation between the launches; every sum over frames or rows: thread i adds elements
// i, i + 256, ... in index order, then a fixed tree over the 256 threads -- the same bits on every run.  The definitions:
// include/tcdiff_hip.h.
//
//   kinetic_features_kernel   one workgroup per (clip, dancer): joints read in place through their element strides; per joint the
//                             windowed velocities / accelerations of the thread's frames and one three-value tree
//   set_moments_kernel        one workgroup per feature column: mean, population std (fit) or the reference's (score); the
//                             normalised column z, its mean mu, the centred column zc, both stored column-major [D][N]
//   set_pairs_kernel          workgroups [0, D ceil(D / 8)): row i of the covariance against eight columns j >= i, mirrored;
//                             workgroups behind them (scores only): one row's distances to every later row
//   set_fid_kernel            ONE workgroup of 512: three D x D matrices in dynamic LDS (leading dimension D | 1: a column walk
//                             touches every bank once); parallel-ordered Jacobi of S1 with eigenvectors, R = V r(w) V^T,
//                             R S2 R, Jacobi of its symmetric part (values only), the traces, and the tree over the distance rows
#include "common.h"
#include "tcdiff_hip.h"

#define TC_SET_THREADS 256
#define TC_SET_TILE 8
#define TC_SET_EIG_THREADS 512
#define TC_SET_MAX_PAIRS ((TC_SET_MAX_D + 1) / 2)

// fixed tree over the workgroup's first 256 threads, NV values at once; every thread calls it and gets the totals
template <int NV>
DEVINL void block_sum_n(double (&x)[NV], double* red) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    __syncthreads();                                      // the previous totals have been read
    if (tid < TC_SET_THREADS) {
#pragma unroll
        for (int v = 0; v < NV; ++v) red[v * TC_SET_THREADS + tid] = x[v];
    }
    __syncthreads();
    for (int o = TC_SET_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int v = 0; v < NV; ++v) red[v * TC_SET_THREADS + tid] = red[v * TC_SET_THREADS + tid] + red[v * TC_SET_THREADS + tid + o];
        }
        __syncthreads();
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) x[v] = red[v * TC_SET_THREADS];
}

DEVINL double set_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// ---- 1. kinetic features ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TC_SET_THREADS) void kinetic_features_kernel(const float* __restrict__ joints, long jsb, long jsd,
                                                                          long jst, int dn, int T, int up, int w, double dt,
                                                                          double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double s_red[3 * TC_SET_THREADS];
    const int tid = threadIdx.x;
    const long q = blockIdx.x;                            // sequence = clip * dn + dancer
    const long c = q / dn;
    const int d = (int)(q - c * dn);
    double* o = out + q * 72;
    if (T < 3) {                                          // an acceleration window would be empty
        if (tid < 72) o[tid] = set_nan();
        return;
    }
    const float* J = joints + c * jsb + d * jsd;
    const double dt2 = dt * dt;
    const int n = T - 1;
    for (int j = 0; j < 24; ++j) {
        const float* Jj = J + 3 * j;
        double acc[3] = {0.0, 0.0, 0.0};
        for (int e = tid; e < n; e += TC_SET_THREADS) {
            const int i = e + 1;
            const int lo = i - w < 1 ? 1 : i - w;         // w <= T (the launcher clamps it)
            const int hi = i + w > T - 1 ? T - 1 : i + w; // the velocity window lo .. hi
            const int ha = i + w > T - 2 ? T - 2 : i + w; // the acceleration window lo .. ha (ha >= lo: T >= 3, w >= 1; ha + 1 >= hi)
            double sv[3] = {0.0, 0.0, 0.0}, sa[3] = {0.0, 0.0, 0.0}, dp[3] = {0.0, 0.0, 0.0};
            const float* P = Jj + (long)(lo - 1) * jst;
            float p0 = P[0], p1 = P[1], p2 = P[2];
            for (int s = lo; s <= ha + 1; ++s) {
                const float* C = Jj + (long)s * jst;
                const float c0 = C[0], c1 = C[1], c2 = C[2];
                const double dc[3] = {(double)c0 - (double)p0, (double)c1 - (double)p1, (double)c2 - (double)p2};   // exact
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (s <= hi) sv[k] += dc[k];
                    if (s > lo) sa[k] += (dc[k] - dp[k]) / dt2;              // the term of s - 1
                    dp[k] = dc[k];
                }
                p0 = c0; p1 = c1; p2 = c2;
            }
            const double dv = (double)(hi - lo + 1) * dt, na = (double)(ha - lo + 1);
            const double vx = sv[0] / dv, vy = sv[1] / dv, vz = sv[2] / dv;
            const double ax = sa[0] / na, ay = sa[1] / na, az = sa[2] / na;
            const double vu = up == 0 ? vx : (up == 1 ? vy : vz);
            const double vp = up == 0 ? vy : vx, vq = up == 2 ? vy : vz;     // the two flat components, in axis order
            acc[0] += vp * vp + vq * vq;
            acc[1] += vu * vu;
            acc[2] += sqrt((ax * ax + ay * ay) + az * az);
        }
        block_sum_n<3>(acc, s_red);
        if (tid == 0) {
            o[3 * j] = acc[0] / (double)n;
            o[3 * j + 1] = acc[1] / (double)n;
            o[3 * j + 2] = acc[2] / (double)n;
        }
    }
}

// ---- 2. moments of a set -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TC_SET_THREADS) void set_moments_kernel(const double* __restrict__ feats, long N, int D, int fit,
                                                                     double* __restrict__ mean, double* __restrict__ std_,
                                                                     double* __restrict__ z, double* __restrict__ zc,
                                                                     double* __restrict__ mu) {
#pragma clang fp contract(off)
    __shared__ double s_red[TC_SET_THREADS];
    const int tid = threadIdx.x;
    const int c = blockIdx.x;
    const double* x = feats + c;
    double m, sd;
    if (fit) {
        double a[1] = {0.0};
        for (long n = tid; n < N; n += TC_SET_THREADS) a[0] += x[n * D];
        block_sum_n<1>(a, s_red);
        m = a[0] / (double)N;
        a[0] = 0.0;
        for (long n = tid; n < N; n += TC_SET_THREADS) {
            const double e = x[n * D] - m;
            a[0] += e * e;
        }
        block_sum_n<1>(a, s_red);
        sd = sqrt(a[0] / (double)N);
        if (tid == 0) {
            mean[c] = m;
            std_[c] = sd;
        }
    } else {
        m = mean[c];
        sd = std_[c];
    }
    const double den = sd + 1e-10;
    double* zcol = z + (long)c * N;
    double* zccol = zc + (long)c * N;
    double a[1] = {0.0};
    for (long n = tid; n < N; n += TC_SET_THREADS) {
        const double v = (x[n * D] - m) / den;
        zcol[n] = v;
        a[0] += v;
    }
    block_sum_n<1>(a, s_red);
    const double mz = a[0] / (double)N;
    if (tid == 0) mu[c] = mz;
    for (long n = tid; n < N; n += TC_SET_THREADS) zccol[n] = zcol[n] - mz;      // the thread's own stores
}

// ---- 3. covariance tiles and distance rows -----------------------------------------------------------------------------------
__global__ __launch_bounds__(TC_SET_THREADS) void set_pairs_kernel(const double* __restrict__ z, const double* __restrict__ zc,
                                                                   long N, int D, int n_cov, double* __restrict__ cov,
                                                                   double* __restrict__ div_rows) {
#pragma clang fp contract(off)
    __shared__ double s_red[TC_SET_TILE * TC_SET_THREADS];
    __shared__ double s_zi[TC_SET_MAX_D];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < n_cov) {
        const int ntile = (D + TC_SET_TILE - 1) / TC_SET_TILE;
        const int i = blockIdx.x / ntile, j0 = (blockIdx.x - i * ntile) * TC_SET_TILE;
        if (j0 + TC_SET_TILE - 1 < i) return;             // the whole tile lies below the diagonal: its mirror writes it
        const double* zi = zc + (long)i * N;
        double acc[TC_SET_TILE];
#pragma unroll
        for (int k = 0; k < TC_SET_TILE; ++k) acc[k] = 0.0;
        for (long n = tid; n < N; n += TC_SET_THREADS) {
            const double a = zi[n];
#pragma unroll
            for (int k = 0; k < TC_SET_TILE; ++k) {
                const int j = j0 + k;
                if (j >= i && j < D) acc[k] += a * zc[(long)j * N + n];
            }
        }
        block_sum_n<TC_SET_TILE>(acc, s_red);
        if (tid < TC_SET_TILE) {
            const int j = j0 + tid;
            if (j >= i && j < D) {
                const double v = acc[tid] / (double)(N - 1);
                cov[(long)i * D + j] = v;
                cov[(long)j * D + i] = v;
            }
        }
        return;
    }
    const long i = (long)blockIdx.x - n_cov;               // distances of row i to the rows behind it
    for (int k = tid; k < D; k += TC_SET_THREADS) s_zi[k] = z[(long)k * N + i];
    __syncthreads();
    double acc[1] = {0.0};
    for (long j = i + 1 + tid; j < N; j += TC_SET_THREADS) {
        double s = 0.0;
        for (int k = 0; k < D; ++k) {
            const double e = s_zi[k] - z[(long)k * N + j];
            s += e * e;
        }
        acc[0] += sqrt(s);
    }
    block_sum_n<1>(acc, s_red);
    if (tid == 0) div_rows[i] = acc[0];
}

// ---- 4. the Frechet distance ---------------------------------------------------------------------------------------------------
struct jacobi_step {                                      // one step's disjoint rotations, written by the pairs' threads
    int p[TC_SET_MAX_PAIRS], q[TC_SET_MAX_PAIRS], on[TC_SET_MAX_PAIRS];
    double c[TC_SET_MAX_PAIRS], s[TC_SET_MAX_PAIRS];
    int rotations;
};

// Symmetric A (D x D, leading dimension ld) -> its eigenvalues on the diagonal; V (or NULL) must come in as the identity and leaves
// with the eigenvectors in its columns.  Round-robin ordering: m = D rounded up to even players, m - 1 steps of m / 2 disjoint
// pairs per sweep (a pair with the padding player is idle).  Returns the number of sweeps, the last one without a rotation, or -1
// when max_sweeps sweeps all rotated.  Every thread of the workgroup calls it.
DEVINL int jacobi_sweeps(double* A, double* V, int D, int ld, int max_sweeps, jacobi_step* st) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const int m = (D + 1) & ~1, np = m / 2;
    for (int sweep = 1; sweep <= max_sweeps; ++sweep) {
        if (tid == 0) st->rotations = 0;
        for (int r = 0; r < m - 1; ++r) {
            __syncthreads();                              // the previous step is complete
            int p = 0, q = 0, on = 0;
            double dpp = 0.0, dqq = 0.0;
            if (tid < np) {
                const int a = tid == 0 ? m - 1 : (r + tid) % (m - 1);
                const int b = tid == 0 ? r : (r - tid + (m - 1)) % (m - 1);
                p = a < b ? a : b;
                q = a < b ? b : a;
                double c = 1.0, s = 0.0;
                if (q < D) {
                    const double apq = A[p * ld + q], app = A[p * ld + p], aqq = A[q * ld + q];
                    if (fabs(apq) > 0x1p-60 * sqrt(fabs(app * aqq))) {       // (a NaN compares false: no rotation)
                        const double theta = (aqq - app) / (2.0 * apq);
                        const double t0 = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                        const double t = theta < 0.0 ? -t0 : t0;
                        c = 1.0 / sqrt(t * t + 1.0);
                        s = t * c;
                        dpp = app - t * apq;
                        dqq = aqq + t * apq;
                        on = 1;
                    }
                }
                st->p[tid] = p;
                st->q[tid] = q;
                st->on[tid] = on;
                st->c[tid] = c;
                st->s[tid] = s;
            }
            __syncthreads();
            for (int idx = tid; idx < np * D; idx += TC_SET_EIG_THREADS) {   // columns: A <- A J, V <- V J
                const int k = idx / D, i = idx - k * D;
                if (!st->on[k]) continue;
                const int cp = st->p[k], cq = st->q[k];
                const double c = st->c[k], s = st->s[k];
                const double x = A[i * ld + cp], y = A[i * ld + cq];
                A[i * ld + cp] = c * x - s * y;
                A[i * ld + cq] = s * x + c * y;
                if (V) {
                    const double vx = V[i * ld + cp], vy = V[i * ld + cq];
                    V[i * ld + cp] = c * vx - s * vy;
                    V[i * ld + cq] = s * vx + c * vy;
                }
            }
            __syncthreads();
            for (int idx = tid; idx < np * D; idx += TC_SET_EIG_THREADS) {   // rows: A <- J^T A
                const int k = idx / D, j = idx - k * D;
                if (!st->on[k]) continue;
                const int rp = st->p[k], rq = st->q[k];
                const double c = st->c[k], s = st->s[k];
                const double x = A[rp * ld + j], y = A[rq * ld + j];
                A[rp * ld + j] = c * x - s * y;
                A[rq * ld + j] = s * x + c * y;
            }
            __syncthreads();
            if (on) {                                     // the rotated 2 x 2 block in closed form: the pair's element is zero
                A[p * ld + p] = dpp;
                A[q * ld + q] = dqq;
                A[p * ld + q] = 0.0;
                A[q * ld + p] = 0.0;
            }
            if (tid == 0) {
                int n = 0;
                for (int k = 0; k < np; ++k) n += st->on[k];
                st->rotations += n;
            }
        }
        __syncthreads();
        const int rotations = st->rotations;
        __syncthreads();                                  // read by everyone before the next sweep clears it
        if (rotations == 0) return sweep;
    }
    return -1;
}

// r(x) of the header for the eigenvalues on A's diagonal, to rt[0 .. D)
DEVINL void clamped_roots(const double* A, int D, int ld, double* rt) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    if (tid < D) {
        double xmax = A[0];
        for (int k = 1; k < D; ++k) xmax = A[k * ld + k] > xmax ? A[k * ld + k] : xmax;
        const double thr = (double)D * 0x1p-52 * (xmax > 0.0 ? xmax : 0.0);
        const double x = A[tid * ld + tid];
        rt[tid] = x > thr ? sqrt(x) : 0.0;
    }
}

__global__ __launch_bounds__(TC_SET_EIG_THREADS) void set_fid_kernel(const double* __restrict__ ref_mu, const double* __restrict__ S1,
                                                                     const double* __restrict__ mu, const double* __restrict__ S2,
                                                                     const double* __restrict__ div_rows, long M, int D,
                                                                     int max_sweeps, double* __restrict__ fid,
                                                                     double* __restrict__ div, int* __restrict__ status) {
#pragma clang fp contract(off)
    extern __shared__ double s_mat[];
    __shared__ jacobi_step s_step;
    __shared__ double s_rt[TC_SET_MAX_D];
    __shared__ double s_red[TC_SET_THREADS];
    const int tid = threadIdx.x;
    const int ld = D | 1;
    double* A = s_mat;
    double* V = s_mat + D * ld;
    double* B = s_mat + 2 * D * ld;

    // div: the tree over the rows' sums
    {
        double a[1] = {0.0};
        if (tid < TC_SET_THREADS)
            for (long i = tid; i < M; i += TC_SET_THREADS) a[0] += div_rows[i];
        block_sum_n<1>(a, s_red);
        if (tid == 0) div[0] = a[0] / ((double)M * (double)(M - 1) / 2.0);
    }

    for (int idx = tid; idx < D * D; idx += TC_SET_EIG_THREADS) {
        const int i = idx / D, j = idx - i * D;
        A[i * ld + j] = S1[idx];
        V[i * ld + j] = i == j ? 1.0 : 0.0;
    }
    const int sweeps1 = jacobi_sweeps(A, V, D, ld, max_sweeps, &s_step);
    __syncthreads();
    clamped_roots(A, D, ld, s_rt);
    __syncthreads();
    for (int idx = tid; idx < D * D; idx += TC_SET_EIG_THREADS) {            // R = V diag(r) V^T, one half mirrored
        const int i = idx / D, j = idx - i * D;
        if (i > j) continue;
        double s = 0.0;
        for (int k = 0; k < D; ++k) s += (V[i * ld + k] * s_rt[k]) * V[j * ld + k];
        B[i * ld + j] = s;
        B[j * ld + i] = s;
    }
    for (int idx = tid; idx < D * D; idx += TC_SET_EIG_THREADS) {
        const int i = idx / D, j = idx - i * D;
        A[i * ld + j] = S2[idx];
    }
    __syncthreads();
    for (int idx = tid; idx < D * D; idx += TC_SET_EIG_THREADS) {            // V = R S2
        const int i = idx / D, j = idx - i * D;
        double s = 0.0;
        for (int k = 0; k < D; ++k) s += B[i * ld + k] * A[k * ld + j];
        V[i * ld + j] = s;
    }
    __syncthreads();
    for (int idx = tid; idx < D * D; idx += TC_SET_EIG_THREADS) {            // A = (R S2) R
        const int i = idx / D, j = idx - i * D;
        double s = 0.0;
        for (int k = 0; k < D; ++k) s += V[i * ld + k] * B[k * ld + j];
        A[i * ld + j] = s;
    }
    __syncthreads();
    for (int idx = tid; idx < D * D; idx += TC_SET_EIG_THREADS) {            // its symmetric part
        const int i = idx / D, j = idx - i * D;
        if (i >= j) continue;
        const double h = (A[i * ld + j] + A[j * ld + i]) * 0.5;
        A[i * ld + j] = h;
        A[j * ld + i] = h;
    }
    const int sweeps2 = jacobi_sweeps(A, nullptr, D, ld, max_sweeps, &s_step);
    __syncthreads();
    clamped_roots(A, D, ld, s_rt);
    __syncthreads();
    if (tid == 0) {                                       // D terms each, in index order
        double dm = 0.0, t1 = 0.0, t2 = 0.0, sr = 0.0;
        for (int k = 0; k < D; ++k) {
            const double e = mu[k] - ref_mu[k];
            dm += e * e;
            t1 += S1[(long)k * D + k];
            t2 += S2[(long)k * D + k];
            sr += s_rt[k];
        }
        const int bad = sweeps1 < 0 || sweeps2 < 0;
        fid[0] = bad ? set_nan() : ((dm + t1) + t2) - 2.0 * sr;
        status[0] = bad;
        status[1] = sweeps1;
        status[2] = sweeps2;
    }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
extern "C" int tcdiff_kinetic_features(const float* joints, const long* joint_strides, int b, int dn, int T, int up, int window,
                                       double fps, double* feats, hipStream_t stream) {
    if (!joints || !joint_strides || !feats) return TC_ERR_ARG;
    if (b < 1 || dn < 1 || T < 1 || up < 0 || up > 2 || window < 1 || !(fps > 0.0)) return TC_ERR_ARG;
    const long Q = (long)b * dn;
    if (Q > 0x7fffffffL) return TC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(kinetic_features_kernel, dim3((unsigned)Q), dim3(TC_SET_THREADS), 0, stream, joints, joint_strides[0],
                       joint_strides[1], joint_strides[2], dn, T, up, window < T ? window : T, 1.0 / fps, feats);
    TC_CHECK_LAUNCH();
    return TC_OK;
}

extern "C" int tcdiff_set_stats(const double* feats, long N, int D, int fit, double* mean, double* std_, double* z, double* zc,
                                double* mu, double* cov, double* div_rows, hipStream_t stream) {
    if (!feats || !mean || !std_ || !z || !zc || !mu || !cov) return TC_ERR_ARG;
    if (N < 2 || D < 1) return TC_ERR_ARG;
    if (D > TC_SET_MAX_D) return TC_ERR_UNSUPPORTED;
    const int n_cov = D * ((D + TC_SET_TILE - 1) / TC_SET_TILE);
    if (N > 0x7fffffffL - n_cov) return TC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(set_moments_kernel, dim3((unsigned)D), dim3(TC_SET_THREADS), 0, stream, feats, N, D, fit ? 1 : 0, mean, std_,
                       z, zc, mu);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(set_pairs_kernel, dim3((unsigned)(n_cov + (div_rows ? N : 0))), dim3(TC_SET_THREADS), 0, stream, z, zc, N, D,
                       n_cov, cov, div_rows);
    TC_CHECK_LAUNCH();
    return TC_OK;
}

extern "C" int tcdiff_set_scores(const double* ref_mu, const double* ref_cov, const double* mu, const double* cov,
                                 const double* div_rows, long M, int D, int max_sweeps, double* fid, double* div, int* status,
                                 hipStream_t stream) {
    if (!ref_mu || !ref_cov || !mu || !cov || !div_rows || !fid || !div || !status) return TC_ERR_ARG;
    if (M < 2 || D < 1 || max_sweeps < 1 || max_sweeps > TC_SET_MAX_SWEEPS) return TC_ERR_ARG;
    if (D > TC_SET_MAX_D) return TC_ERR_UNSUPPORTED;
    constexpr int max_bytes = 3 * TC_SET_MAX_D * (TC_SET_MAX_D | 1) * (int)sizeof(double);
    static tc_dev_state dev_state;
    const int n_cu = tc_device_once(dev_state, [](int) {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(set_fid_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, max_bytes);
    });
    if (n_cu < 0) return n_cu;
    const int bytes = 3 * D * (D | 1) * (int)sizeof(double);
    hipLaunchKernelGGL(set_fid_kernel, dim3(1), dim3(TC_SET_EIG_THREADS), bytes, stream, ref_mu, ref_cov, mu, cov, div_rows, M, D,
                       max_sweeps, fid, div, status);
    TC_CHECK_LAUNCH();
    return TC_OK;
}

extern "C" int tcdiff_set_check(const int* status, hipStream_t stream) {
    if (!status) return TC_ERR_ARG;
    int h[3] = {0, 0, 0};
    if (hipMemcpyAsync(h, status, sizeof(h), hipMemcpyDeviceToHost, stream) != hipSuccess) return TC_ERR_LAUNCH;
    if (hipStreamSynchronize(stream) != hipSuccess) return TC_ERR_LAUNCH;
    return h[0] ? TC_ERR_NOCONVERGE : TC_OK;
}
