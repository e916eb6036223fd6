// The arithmetic of the group metrics (include/tcdiff_group.h): the distance of two segments, the orientation test of two floor
// steps, a joint's speed and one term of the correlation, as plain functions (no memory traffic of their own, no HIP builtins), so
// that the same source compiles
//   * as __device__ code into libtcdiff_gfx950.so (csrc/group.hip), and
//   * as host code under g++ (tests/host/group_host.cpp), checked on the CPU against the numpy restatement
//     (tests/test_group_cpu.py) before it ever runs on a GPU.
// float64 arithmetic on the float32 inputs, contraction off in every function (g++: build with -ffp-contract=off).
#pragma once
#include <math.h>

#ifndef TC_HD
#if defined(__HIPCC__)
#define TC_HD __host__ __device__ __forceinline__
#else
#define TC_HD static inline
#endif
#endif
#if defined(__clang__)
#define TCG_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TCG_NO_CONTRACT
#endif

#define TCG_J 24                          // joints of a dancer; bones are 1 .. 23
#define TCG_BONE_PAIRS 529                // 23 x 23
#define TCG_SMALL 1e-18                   // a squared length at or below it is a point

struct TcgV { double x, y, z; };
struct TcgBest { double v; int code; };   // a candidate of a minimum and what attains it

TC_HD TcgV tcg_v(double x, double y, double z) { TcgV r; r.x = x; r.y = y; r.z = z; return r; }
TC_HD TcgV tcg_sub(TcgV a, TcgV b) { TCG_NO_CONTRACT return tcg_v(a.x - b.x, a.y - b.y, a.z - b.z); }
TC_HD double tcg_dot(TcgV a, TcgV b) { TCG_NO_CONTRACT return (a.x * b.x + a.y * b.y) + a.z * b.z; }
TC_HD double tcg_norm(TcgV a) { return sqrt(tcg_dot(a, a)); }
TC_HD TcgV tcg_at(TcgV p, double s, TcgV d) { TCG_NO_CONTRACT return tcg_v(p.x + s * d.x, p.y + s * d.y, p.z + s * d.z); }
TC_HD double tcg_clamp(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }          // a NaN passes through

// the distance of the segments p1 -> q1 and p2 -> q2
TC_HD double tcg_seg_dist(TcgV p1, TcgV q1, TcgV p2, TcgV q2) {
    TCG_NO_CONTRACT
    const TcgV d1 = tcg_sub(q1, p1), d2 = tcg_sub(q2, p2), r = tcg_sub(p1, p2);
    const double A = tcg_dot(d1, d1), E = tcg_dot(d2, d2), F = tcg_dot(d2, r);
    double s, u;
    if (A <= TCG_SMALL && E <= TCG_SMALL) {
        s = 0.0;
        u = 0.0;
    } else if (A <= TCG_SMALL) {
        s = 0.0;
        u = tcg_clamp(F / E);
    } else {
        const double C = tcg_dot(d1, r);
        if (E <= TCG_SMALL) {
            u = 0.0;
            s = tcg_clamp(-C / A);
        } else {
            const double B = tcg_dot(d1, d2);
            const double den = A * E - B * B;
            s = den > 0.0 ? tcg_clamp((B * F - C * E) / den) : 0.0;
            u = (B * s + F) / E;
            if (u < 0.0) {
                u = 0.0;
                s = tcg_clamp(-C / A);
            } else if (u > 1.0) {
                u = 1.0;
                s = tcg_clamp((B - C) / A);
            }
        }
    }
    return tcg_norm(tcg_sub(tcg_at(p1, s, d1), tcg_at(p2, u, d2)));
}

// the gap of two capsules
TC_HD double tcg_gap(double dist, double ri, double rj) { TCG_NO_CONTRACT return (dist - ri) - rj; }

// the order of a minimum with its argument: a NaN precedes every number, then the smaller value, then the smaller code
TC_HD int tcg_before(TcgBest a, TcgBest b) {
    const int an = a.v != a.v, bn = b.v != b.v;
    if (an != bn) return an;
    if (an) return a.code < b.code;
    return a.v < b.v || (a.v == b.v && a.code < b.code);
}

// the same for the minimum over the frames, where only finite values take part: code < 0 marks "none yet"
TC_HD int tcg_finite(double v) { return v - v == 0.0; }
TC_HD int tcg_before_finite(TcgBest a, TcgBest b) {
    if (a.code < 0 || b.code < 0) return b.code < 0 && a.code >= 0;
    return a.v < b.v || (a.v == b.v && a.code < b.code);
}

// the two floor coordinates of a joint: the components that are not `up`, in axis order
TC_HD void tcg_floor(const float* j, int up, double* x, double* y) {
    *x = (double)(up == 0 ? j[1] : j[0]);
    *y = (double)(up == 2 ? j[1] : j[2]);
}
TC_HD double tcg_orient(double x0, double x1, double y0, double y1, double z0, double z1) {
    TCG_NO_CONTRACT
    return (y0 - x0) * (z1 - x1) - (y1 - x1) * (z0 - x0);
}
// do the steps a0 -> a1 and b0 -> b1 cross properly?  a[4] = (a0x, a0y, a1x, a1y)
TC_HD int tcg_cross(const double* a, const double* b) {
    TCG_NO_CONTRACT
    const double o1 = tcg_orient(a[0], a[1], a[2], a[3], b[0], b[1]), o2 = tcg_orient(a[0], a[1], a[2], a[3], b[2], b[3]);
    const double o3 = tcg_orient(b[0], b[1], b[2], b[3], a[0], a[1]), o4 = tcg_orient(b[0], b[1], b[2], b[3], a[2], a[3]);
    return o1 * o2 < 0.0 && o3 * o4 < 0.0;
}

// the speed signal of joint j between two frames (J0 at t, J1 at t + 1; 24 x 3 floats each): root-relative for j >= 1
TC_HD double tcg_speed(const float* J0, const float* J1, int j) {
    TCG_NO_CONTRACT
    double d[3];
    for (int k = 0; k < 3; ++k) {
        if (j == 0)
            d[k] = (double)J1[k] - (double)J0[k];
        else
            d[k] = ((double)J1[3 * j + k] - (double)J1[k]) - ((double)J0[3 * j + k] - (double)J0[k]);
    }
    return sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
}

TC_HD double tcg_standard(double x, double mu, double sigma) { TCG_NO_CONTRACT return (x - mu) / sigma; }
// one term of the correlation added to its sum
TC_HD double tcg_corr_add(double sum, double za, double zb) { TCG_NO_CONTRACT return sum + za * zb; }

// the lags that are evaluated: |l| <= tcg_lags(T, max_lag), or none if that is negative
TC_HD int tcg_lags(int T, int max_lag) {
    const int N = T - 1;
    if (N < 2) return -1;
    return max_lag < N - 2 ? max_lag : N - 2;
}
// does (R, lag) beat the best so far?  the larger value, then the smaller |lag|, then the negative lag
TC_HD int tcg_better_lag(double R, int lag, double best, int best_lag) {
    if (R != best) return R > best;
    const int a = lag < 0 ? -lag : lag, b = best_lag < 0 ? -best_lag : best_lag;
    if (a != b) return a < b;
    return lag < best_lag;
}
