// The arithmetic of the choreography planner (include/tcdiff_choreo.h): the PCHIP slopes of a dancer's waypoints, the segment of a
// frame, the Hermite value, the normalised and clamped x_0 channel, the step between two stored frames and the two total orders, as
// plain functions (no memory traffic of their own beyond the rows they are handed, no HIP builtins), so that the same source compiles
//   * as __device__ code into libtcdiff_gfx950.so (csrc/choreo.hip), and
//   * as host code under g++ (tests/host/choreo_host.cpp), checked on the CPU against the numpy restatement
//     (tests/test_choreo_cpu.py) before it ever runs on a GPU.
// float64 arithmetic on the float32 and int32 inputs, contraction off in every function (g++: build with -ffp-contract=off).
// csrc/footlock_math.h supplies TC_HD and TCK_NO_CONTRACT, unchanged.
#pragma once
#include "footlock_math.h"

TC_HD int tcc_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }          // false for a NaN
TC_HD int tcc_sign(double v) { return (v > 0.0) - (v < 0.0); }

// the secant of segment k: (y[k+1] - y[k]) / (key[k+1] - key[k])
TC_HD double tcc_secant(const int* key, const double* y, int k) {
    TCK_NO_CONTRACT
    return (y[k + 1] - y[k]) / (double)(key[k + 1] - key[k]);
}

// an interior slope, Fritsch-Butland: m0, h0 of the segment before the key, m1, h1 of the one after it
TC_HD double tcc_slope_interior(double h0, double h1, double m0, double m1) {
    TCK_NO_CONTRACT
    if (tcc_sign(m0) != tcc_sign(m1) || m0 == 0.0 || m1 == 0.0) return 0.0;
    const double w1 = 2.0 * h1 + h0, w2 = h1 + 2.0 * h0;
    return (w1 + w2) / (w1 / m0 + w2 / m1);
}

// an end slope, the three-point formula and its two guards: h0, m0 of the end segment, h1, m1 of its neighbour
TC_HD double tcc_slope_end(double h0, double h1, double m0, double m1) {
    TCK_NO_CONTRACT
    const double d = ((2.0 * h0 + h1) * m0 - h0 * m1) / (h0 + h1);
    if (tcc_sign(d) != tcc_sign(m0)) return 0.0;
    if (tcc_sign(m0) != tcc_sign(m1) && fabs(d) > 3.0 * fabs(m0)) return 3.0 * m0;
    return d;
}

// the slope at key k of `count` keys (strictly ascending) with the values y
TC_HD double tcc_slope(const int* key, const double* y, int count, int k) {
    TCK_NO_CONTRACT
    if (count < 2) return 0.0;
    if (count == 2) return tcc_secant(key, y, 0);
    if (k == 0) return tcc_slope_end((double)(key[1] - key[0]), (double)(key[2] - key[1]), tcc_secant(key, y, 0), tcc_secant(key, y, 1));
    if (k == count - 1)
        return tcc_slope_end((double)(key[k] - key[k - 1]), (double)(key[k - 1] - key[k - 2]), tcc_secant(key, y, k - 1), tcc_secant(key, y, k - 2));
    return tcc_slope_interior((double)(key[k] - key[k - 1]), (double)(key[k + 1] - key[k]), tcc_secant(key, y, k - 1), tcc_secant(key, y, k));
}

// the segment of frame t, key[0] < t < key[count - 1]: the largest k with key[k] <= t
TC_HD int tcc_segment(const int* key, int count, int t) {
    int lo = 0, hi = count - 1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (key[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// one component at frame t: the first point up to the first key, the last from the last key on, the Hermite form between
TC_HD double tcc_eval(const int* key, const double* y, const double* d, int count, int t) {
    TCK_NO_CONTRACT
    if (t <= key[0]) return y[0];
    if (t >= key[count - 1]) return y[count - 1];
    const int k = tcc_segment(key, count, t);
    const double h = (double)(key[k + 1] - key[k]);
    const double s = (double)(t - key[k]) / h, u = 1.0 - s;
    const double h00 = ((1.0 + 2.0 * s) * u) * u, h10 = (s * u) * u, h01 = (s * s) * (3.0 - 2.0 * s), h11 = (s * s) * (s - 1.0);
    return (h00 * y[k] + h10 * (h * d[k])) + (h01 * y[k + 1] + h11 * (h * d[k + 1]));
}

// a channel of x_0: v scale + min, clamped to [-1, 1]; clamped[0] is set when the clamp changed it
TC_HD double tcc_x0(double v, double scale, double mn, int* clamped) {
    TCK_NO_CONTRACT
    const double n = v * scale + mn;
    if (n < -1.0) { *clamped = 1; return -1.0; }
    if (n > 1.0) { *clamped = 1; return 1.0; }
    return n;
}

// the floor distance of two points given as float32
TC_HD double tcc_dist(float ax, float ay, float bx, float by) {
    TCK_NO_CONTRACT
    const double dx = (double)bx - (double)ax, dy = (double)by - (double)ay;
    return sqrt(dx * dx + dy * dy);
}

// running extrema over a total order; t < 0: nothing yet
struct TccPeak { double v; int t; };
TC_HD int tcc_larger(TccPeak a, TccPeak b) {          // the larger value, then the lower frame
    if (a.t < 0) return 0;
    if (b.t < 0) return 1;
    if (a.v != b.v) return a.v > b.v;
    return a.t < b.t;
}
TC_HD int tcc_smaller(TccPeak a, TccPeak b) {         // the smaller value, then the lower frame
    if (a.t < 0) return 0;
    if (b.t < 0) return 1;
    if (a.v != b.v) return a.v < b.v;
    return a.t < b.t;
}
TC_HD int tcc_later(TccPeak a, TccPeak b) {           // the higher frame
    return a.t > b.t;
}

// pair p of dn dancers in the order (0,1), (0,2), ..., (1,2), ...
TC_HD void tcc_pair(int p, int dn, int* i, int* j) {
    int a = 0;
    while (p >= dn - 1 - a) { p -= dn - 1 - a; ++a; }
    *i = a;
    *j = a + 1 + p;
}
