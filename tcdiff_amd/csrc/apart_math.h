// The arithmetic of keeping the dancers apart (include/tcdiff_apart.h): the direction of a pair's push, the moved joints, the body gap
// of two sets of float64 joints over a range of bone pairs, the iteration's step, the envelope's weight and the shifted output, as
// plain functions (no memory traffic of their own, no HIP builtins), so that the same source compiles
//   * as __device__ code into libtcdiff_gfx950.so (csrc/apart.hip), and
//   * as host code under g++ (tests/host/apart_host.cpp), checked on the CPU against the numpy restatement
//     (tests/test_apart_cpu.py) before it ever runs on a GPU.
// The distance, the gap and the order of a minimum are csrc/group_math.h's, unchanged.  float64 arithmetic on the float32 inputs,
// contraction off in every function (g++: build with -ffp-contract=off).
#pragma once
#include "group_math.h"

struct TcpDir { double x, y; };           // a floor vector: the components f0 and f1

// the two floor components of a 3-vector are those that are not `up`; a floor vector as a 3-vector with 0 in the `up` place
TC_HD TcgV tcp_lift(TcpDir d, int up) { return up == 0 ? tcg_v(0.0, d.x, d.y) : (up == 1 ? tcg_v(d.x, 0.0, d.y) : tcg_v(d.x, d.y, 0.0)); }
TC_HD TcpDir tcp_floor(TcgV v, int up) {
    TcpDir r;
    r.x = up == 0 ? v.y : v.x;
    r.y = up == 2 ? v.y : v.z;
    return r;
}

// one coordinate of a staged joint: component k (0 .. 2) of the float32 word x with the shift added to a floor component
TC_HD double tcp_stage(float x, int k, int up, double s0, double s1) {
    TCG_NO_CONTRACT
    if (k == up) return (double)x;
    const int first = k == (up == 0 ? 1 : 0);
    return (double)x + (first ? s0 : s1);
}

// the unit floor vector from root a to root b; (1, 0) if they coincide (or one is NaN)
TC_HD TcpDir tcp_direction(TcpDir ra, TcpDir rb) {
    TCG_NO_CONTRACT
    const double d0 = rb.x - ra.x, d1 = rb.y - ra.y;
    const double n2 = d0 * d0 + d1 * d1;
    TcpDir u;
    if (n2 > TCG_SMALL) {
        const double n = sqrt(n2);
        u.x = d0 / n;
        u.y = d1 / n;
    } else {
        u.x = 1.0;
        u.y = 0.0;
    }
    return u;
}

// the shares of a pair's push; 0 is returned for a pinned pair (both mobilities 0)
TC_HD int tcp_shares(double mob_a, double mob_b, double* wa, double* wb) {
    TCG_NO_CONTRACT
    if (mob_a == 0.0 && mob_b == 0.0) {
        *wa = 0.0;
        *wb = 0.0;
        return 0;
    }
    *wa = mob_a / (mob_a + mob_b);
    *wb = 1.0 - *wa;
    return 1;
}

// what a joint of a (sign -1) or of b (sign +1) moves by at push m: (w m) u, lifted
TC_HD TcgV tcp_move(double w, double m, TcpDir u, int up) {
    TCG_NO_CONTRACT
    const double q = w * m;
    TcpDir d;
    d.x = q * u.x;
    d.y = q * u.y;
    return tcp_lift(d, up);
}
TC_HD TcgV tcp_joint(const double* J, int j) { return tcg_v(J[3 * j], J[3 * j + 1], J[3 * j + 2]); }
TC_HD TcgV tcp_add(TcgV a, TcgV b) { TCG_NO_CONTRACT return tcg_v(a.x + b.x, a.y + b.y, a.z + b.z); }

// the smallest (gap, code) of the bone pairs k = first, first + step, ... < 529 of Ja - da and Jb + db (24 x 3 float64 each), in
// tcdiff_group.h's order; code -1 if the range is empty
TC_HD TcgBest tcp_gap_range(const double* Ja, const double* Jb, TcgV da, TcgV db, const int* parents, const double* radii, int first, int step) {
    TcgBest best;
    best.v = 0.0;
    best.code = -1;
    for (int k = first; k < TCG_BONE_PAIRS; k += step) {
        const int i = 1 + k / 23, j = 1 + k % 23;
        const int pi = parents[i], pj = parents[j];
        const double d = tcg_seg_dist(tcg_sub(tcp_joint(Ja, pi), da), tcg_sub(tcp_joint(Ja, i), da), tcp_add(tcp_joint(Jb, pj), db),
                                      tcp_add(tcp_joint(Jb, j), db));
        TcgBest cand;
        cand.v = tcg_gap(d, radii[i], radii[j]);
        cand.code = TCG_J * i + j;
        if (best.code < 0 || tcg_before(cand, best)) best = cand;
    }
    return best;
}

// one step of the iteration: 0 = stop (m as it is; a NaN gap: m = 0), 1 = evaluate g(m) and go on, 2 = evaluate g(m), capped, stop
TC_HD int tcp_step(double g, double margin, double max_push, double* m) {
    TCG_NO_CONTRACT
    if (g != g) {
        *m = 0.0;
        return 0;
    }
    const double need = margin - g;
    if (!(need > 0.0)) return 0;
    const double next = *m + need;
    *m = next < max_push ? next : max_push;
    return *m == max_push ? 2 : 1;
}

// the envelope's candidate of a frame k frames away
TC_HD double tcp_tent(double m, int k, int blend) {
    TCG_NO_CONTRACT
    return m * (1.0 - (double)k / ((double)blend + 1.0));
}

// S -/+ (w e) u, component by component: sign -1 for a, +1 for b
TC_HD TcpDir tcp_shift(TcpDir S, double w, double e, TcpDir u, int sign) {
    TCG_NO_CONTRACT
    const double q = w * e;
    TcpDir r;
    r.x = sign < 0 ? S.x - q * u.x : S.x + q * u.x;
    r.y = sign < 0 ? S.y - q * u.y : S.y + q * u.y;
    return r;
}

// an output word: float32(float64(x) + s)
TC_HD float tcp_out(float x, double s) { TCG_NO_CONTRACT return (float)((double)x + s); }
TC_HD double tcp_length(double x, double y) { TCG_NO_CONTRACT return sqrt(x * x + y * y); }
