// The arithmetic of the beat synchroniser (include/tcdiff_beatsync.h): the speed of a frame, the reflected Gaussian sum, the minima,
// the nearest kinematic beat of a music beat and whether it keeps its claim, the serial anchor pass, the warp of a frame, the source
// frame of an output frame, the root's interpolation and a joint's slerp, as plain functions (no memory traffic of their own beyond
// the rows they are handed, no HIP builtins), so that the same source compiles
//   * as __device__ code into libtcdiff_gfx950.so (csrc/beatsync.hip), and
//   * as host code under g++ (tests/host/beatsync_host.cpp), checked on the CPU against the numpy restatement
//     (tests/test_beatsync_cpu.py) before it ever runs on a GPU.
// float64 arithmetic on the float32 and int32 inputs, contraction off in every function (g++: build with -ffp-contract=off).
// csrc/choreo_math.h supplies the PCHIP slopes and the Hermite value on float64 values (tcc_slope, tcc_eval) and the total orders,
// csrc/footlock_math.h the quaternions (tck_quat, tck_rotvec), both unchanged.
#pragma once
#include "choreo_math.h"

#define TCB_J 24
#define TCB_LINEAR 0.01                   // 1 - d below it: the linear weights of stitch.quat_slerp

TC_HD int tcb_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }          // false for a NaN
TC_HD int tcb_finite3(const float* p) { return tcb_finite((double)p[0]) && tcb_finite((double)p[1]) && tcb_finite((double)p[2]); }

// v of a frame: J0 and J1 are the 24 x 3 joints of frames t and t + 1
TC_HD double tcb_speed(const float* J0, const float* J1) {
    TCK_NO_CONTRACT
    double sum = 0.0;
    for (int j = 0; j < TCB_J; ++j) {
        const double dx = (double)J1[3 * j] - (double)J0[3 * j], dy = (double)J1[3 * j + 1] - (double)J0[3 * j + 1],
                     dz = (double)J1[3 * j + 2] - (double)J0[3 * j + 2];
        sum = sum + sqrt((dx * dx + dy * dy) + dz * dz);
    }
    return sum / 24.0;
}

// the non-finite mask of a frame's pose: bit j for joint j, bit 24 for the root
TC_HD unsigned tcb_mask(const float* q, const float* pos) {
    unsigned m = 0;
    for (int j = 0; j < TCB_J; ++j)
        if (!tcb_finite3(q + 3 * j)) m |= 1u << j;
    if (!tcb_finite3(pos)) m |= 1u << TCB_J;
    return m;
}

// "reflect": (d c b a | a b c d | d c b a), period 2 N, whatever the distance from the array; N >= 1
TC_HD int tcb_reflect(int i, int N) {
    if (i >= 0 && i < N) return i;
    const int per = 2 * N;
    i %= per;
    if (i < 0) i += per;
    return i >= N ? per - 1 - i : i;
}

// s[t]: pv [N], w [2 rad + 1], ascending taps to 0.0
TC_HD double tcb_filter(const double* pv, int N, const double* w, int rad, int t) {
    TCK_NO_CONTRACT
    double acc = 0.0;
    for (int x = -rad; x <= rad; ++x) acc = acc + w[x + rad] * pv[tcb_reflect(t + x, N)];
    return acc;
}

// a strict interior local minimum of s [N]
TC_HD int tcb_is_min(const double* s, int N, int t) { return t >= 1 && t <= N - 2 && s[t] < s[t - 1] && s[t] < s[t + 1]; }

// the index in the ascending list [n] of the entry nearest to m, the lower one of two at the same distance; -1 for an empty list
TC_HD int tcb_nearest(const int* list, int n, int m) {
    if (n < 1) return -1;
    int lo = 0, hi = n;                                       // the first entry >= m
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < m) lo = mid + 1; else hi = mid;
    }
    if (lo == 0) return 0;
    if (lo == n) return n - 1;
    return m - list[lo - 1] <= list[lo] - m ? lo - 1 : lo;
}

// music beat i of mus [nm] picked kin[pick[i]] (pick[i] < 0: none within max_shift).  Does it keep its claim?  The claimants of one
// kinematic beat are neighbours in the list: the smaller distance wins, then the lower m.
TC_HD int tcb_keeps(const int* mus, const int* pick, const int* kin, int nm, int i) {
    const int p = pick[i];
    if (p < 0) return 0;
    const int k = kin[p], m = mus[i];
    const int mine = m < k ? k - m : m - k;
    for (int o = i - 1; o >= 0 && pick[o] == p; --o) {        // lower m: wins at an equal distance
        const int d = mus[o] < k ? k - mus[o] : mus[o] - k;
        if (d <= mine) return 0;
    }
    for (int o = i + 1; o < nm && pick[o] == p; ++o) {
        const int d = mus[o] < k ? k - mus[o] : mus[o] - k;
        if (d < mine) return 0;
    }
    return 1;
}

TC_HD int tcb_rate_ok(double r, double lo, double hi) { return r >= lo && r <= hi; }

// the serial pass: candidates (cm, ck) [nc] in ascending m -> keys am, values au and shifts ae [count], count = kept + 2; dropped[0] is set
TC_HD int tcb_anchor_pass(const int* cm, const int* ck, int nc, int T, double strength, double max_rate, int* am, double* au, double* ae,
                          int* dropped) {
    TCK_NO_CONTRACT
    const double lo = 1.0 / max_rate, end = (double)(T - 1);
    int n = 1, drop = 0;
    am[0] = 0;
    au[0] = 0.0;
    ae[0] = 0.0;
    for (int i = 0; i < nc; ++i) {
        const double e = strength * (double)(ck[i] - cm[i]);
        const double u = (double)cm[i] + e;
        const double r = (u - au[n - 1]) / (double)(cm[i] - am[n - 1]);
        if (tcb_rate_ok(r, lo, max_rate)) {
            am[n] = cm[i];
            au[n] = u;
            ae[n] = e;
            ++n;
        } else {
            ++drop;
        }
    }
    while (n > 1 && !tcb_rate_ok((end - au[n - 1]) / (double)((T - 1) - am[n - 1]), lo, max_rate)) {
        --n;
        ++drop;
    }
    am[n] = T - 1;
    au[n] = end;
    ae[n] = 0.0;
    *dropped = drop;
    return n + 1;
}

// warp[t], the cubic about the diagonal: ae the shifts, ad1 the slopes minus 1; count == 2 is the identity, exactly
TC_HD double tcb_warp(const int* am, const double* ae, const double* ad1, int count, int T, int t) {
    TCK_NO_CONTRACT
    if (count <= 2) return (double)t;
    const double w = (double)t + tcc_eval(am, ae, ad1, count, t), end = (double)(T - 1);
    return w < 0.0 ? 0.0 : (w > end ? end : w);
}

// the source frame i and the weight a of a source time 0 <= u <= T - 1
TC_HD int tcb_source(double u, int T, double* a) {
    TCK_NO_CONTRACT
    int i = (int)floor(u);
    i = i < 0 ? 0 : (i > T - 1 ? T - 1 : i);
    *a = u - (double)i;
    return i;
}

TC_HD double tcb_lerp(float p0, float p1, double a) {
    TCK_NO_CONTRACT
    return (1.0 - a) * (double)p0 + a * (double)p1;
}

// a joint between two frames: the rotation vectors qa, qb (three float32 each, all finite), 0 < a < 1
TC_HD TckV tcb_slerp(const float* qa, const float* qb, double a) {
    TCK_NO_CONTRACT
    const TckQ A = tck_quat(qa);
    TckQ B = tck_quat(qb);
    double d = ((A.w * B.w + A.x * B.x) + A.y * B.y) + A.z * B.z;
    if (d < 0.0) {
        d = -d;
        B = tck_q(-B.w, -B.x, -B.y, -B.z);
    }
    double w0 = 1.0 - a, w1 = a;
    if (!(1.0 - d < TCB_LINEAR)) {
        const double om = acos(d), so = sin(om);
        w0 = sin((1.0 - a) * om) / so;
        w1 = sin(a * om) / so;
    }
    const double rw = w0 * A.w + w1 * B.w, rx = w0 * A.x + w1 * B.x, ry = w0 * A.y + w1 * B.y, rz = w0 * A.z + w1 * B.z;
    const double n = sqrt(((rw * rw + rx * rx) + ry * ry) + rz * rz);
    return tck_rotvec(tck_q(rw / n, rx / n, ry / n, rz / n));
}
