// The arithmetic of the jitter scores and of the rotation filter (include/tcdiff_smooth.h): the window of a frame, the tap sums of the
// root and of a joint's quaternions with the sign rule, the change between two rotation vectors, and the acceleration and jerk terms,
// as plain functions (no memory traffic of their own beyond the rows they are handed, no HIP builtins), so that the same source compiles
//   * as __device__ code into libtcdiff_gfx950.so (csrc/smooth.hip), and
//   * as host code under g++ (tests/host/smooth_host.cpp), checked on the CPU against the numpy restatement
//     (tests/test_smooth_cpu.py) before it ever runs on a GPU.
// float64 arithmetic on the float32 inputs, contraction off in every function (g++: build with -ffp-contract=off).
// csrc/footlock_math.h supplies the vectors and quaternions (tck_quat, tck_rotvec, tck_mul), unchanged.
#pragma once
#include "footlock_math.h"

#define TCW_J 24
#define TCW_MIN_NORM 1e-6                 // a filtered quaternion shorter than this has no direction: the joint is copied through

TC_HD int tcw_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }          // false for a NaN

// the first frame of the window of frame t: W frames, centred where it can be
TC_HD int tcw_start(int t, int T, int W) {
    const int s = t - (W - 1) / 2;
    return s < 0 ? 0 : (s > T - W ? T - W : s);
}

// one component of the root: x[0 .. W) are the window's values, tap the row of the table
TC_HD double tcw_tap_sum(const double* tap, const double* x, int W) {
    TCK_NO_CONTRACT
    double acc = 0.0;
    for (int u = 0; u < W; ++u) acc = acc + tap[u] * x[u];
    return acc;
}

struct TcwRot { int copied; TckV r; };          // r is set when copied == 0

// one joint: Q + c cs + u is component c (w, x, y, z) of the quaternion of the window's frame u; `self` is the output frame's place
// in the window
TC_HD TcwRot tcw_filter_quat(const double* tap, const double* Q, long cs, int W, int self) {
    TCK_NO_CONTRACT
    const double sw = Q[self], sx = Q[cs + self], sy = Q[2 * cs + self], sz = Q[3 * cs + self];
    double aw = 0.0, ax = 0.0, ay = 0.0, az = 0.0;
    for (int u = 0; u < W; ++u) {
        const double w = Q[u], x = Q[cs + u], y = Q[2 * cs + u], z = Q[3 * cs + u];
        const double dot = ((sw * w + sx * x) + sy * y) + sz * z;
        const double k = dot < 0.0 ? -tap[u] : tap[u];
        aw = aw + k * w;
        ax = ax + k * x;
        ay = ay + k * y;
        az = az + k * z;
    }
    const double n = sqrt(((aw * aw + ax * ax) + ay * ay) + az * az);
    TcwRot out;
    out.r = tck_v(0.0, 0.0, 0.0);
    out.copied = !(n >= TCW_MIN_NORM);          // a non-finite float in the window makes every component of its quaternion, and so n, NaN
    if (!out.copied) out.r = tck_rotvec(tck_q(aw / n, ax / n, ay / n, az / n));
    return out;
}

// the relative rotation angle of two rotation vectors (three float32 each)
TC_HD double tcw_rot_change(const float* a, const float* b) {
    TCK_NO_CONTRACT
    const TckQ d = tck_mul(tck_conj(tck_quat(a)), tck_quat(b));
    return 2.0 * atan2(tck_norm(tck_v(d.x, d.y, d.z)), fabs(d.w));
}

TC_HD TckV tcw_point(const float* p) { return tck_v((double)p[0], (double)p[1], (double)p[2]); }

// |(p[t+1] - 2 p[t]) + p[t-1]| f2
TC_HD double tcw_accel(TckV pm, TckV p0, TckV p1, double f2) {
    TCK_NO_CONTRACT
    return tck_norm(tck_add(tck_sub(p1, tck_scale(p0, 2.0)), pm)) * f2;
}
// |((p[t+2] - 3 p[t+1]) + 3 p[t]) - p[t-1]| f3
TC_HD double tcw_jerk(TckV pm, TckV p0, TckV p1, TckV p2, double f3) {
    TCK_NO_CONTRACT
    return tck_norm(tck_sub(tck_add(tck_sub(p2, tck_scale(p1, 3.0)), tck_scale(p0, 3.0)), pm)) * f3;
}

// a running maximum over the total order: the larger value, then the lower frame, then the lower joint; t < 0: nothing yet
struct TcwPeak { double v; int t, j; };
TC_HD int tcw_beats(TcwPeak a, TcwPeak b) {
    if (a.t < 0) return 0;
    if (b.t < 0) return 1;
    if (a.v != b.v) return a.v > b.v;
    if (a.t != b.t) return a.t < b.t;
    return a.j < b.j;
}
