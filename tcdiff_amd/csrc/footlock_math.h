// The per-frame arithmetic of the foot lock (include/tcdiff_footlock.h): the float64 chain down one leg, the eased shift of a frame
// outside the runs, the reach clamp, the two-bone solve and the way back to rotation vectors, as plain functions (no memory traffic of
// their own, no HIP builtins), so that the same source compiles
//   * as __device__ code into libtcdiff_gfx950.so (csrc/footlock.hip), and
//   * as host code under g++ (tests/host/footlock_host.cpp), checked on the CPU against the numpy restatement
//     (tests/test_footlock_cpu.py) before it ever runs on a GPU.
// float64 arithmetic on the float32 inputs, contraction off in every function (g++: build with -ffp-contract=off).  Nothing here
// takes the address of a local array: every value is a struct of doubles that lives in registers.
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
#define TCK_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TCK_NO_CONTRACT
#endif

#define TCK_SMALL 1e-3                    // below it the series of sin(theta / 2) / theta, as csrc/gltf_math.h
#define TCK_TINY 1e-9                     // a vector shorter than this has no direction
#define TCK_PI 3.14159265358979323846

struct TckV { double x, y, z; };
struct TckQ { double w, x, y, z; };

TC_HD TckV tck_v(double x, double y, double z) { TckV r; r.x = x; r.y = y; r.z = z; return r; }
TC_HD TckQ tck_q(double w, double x, double y, double z) { TckQ r; r.w = w; r.x = x; r.y = y; r.z = z; return r; }
TC_HD TckV tck_add(TckV a, TckV b) { TCK_NO_CONTRACT return tck_v(a.x + b.x, a.y + b.y, a.z + b.z); }
TC_HD TckV tck_sub(TckV a, TckV b) { TCK_NO_CONTRACT return tck_v(a.x - b.x, a.y - b.y, a.z - b.z); }
TC_HD TckV tck_scale(TckV a, double s) { TCK_NO_CONTRACT return tck_v(a.x * s, a.y * s, a.z * s); }
TC_HD TckV tck_over(TckV a, double s) { TCK_NO_CONTRACT return tck_v(a.x / s, a.y / s, a.z / s); }
TC_HD double tck_dot(TckV a, TckV b) { TCK_NO_CONTRACT return (a.x * b.x + a.y * b.y) + a.z * b.z; }
TC_HD double tck_norm(TckV a) { return sqrt(tck_dot(a, a)); }
TC_HD TckV tck_cross(TckV a, TckV b) {
    TCK_NO_CONTRACT
    return tck_v(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
TC_HD int tck_is_zero(TckV a) { return a.x == 0.0 && a.y == 0.0 && a.z == 0.0; }

// sin(theta / 2) / theta, with the series of csrc/gltf_math.h below TCK_SMALL
TC_HD double tck_half_sinc(double theta) {
    TCK_NO_CONTRACT
    const double a2 = theta * theta;
    return theta < TCK_SMALL ? (0.5 - a2 / 48.0) + a2 * a2 / 3840.0 : sin(theta / 2.0) / theta;
}
// rotation vector (three float32) -> unit quaternion, as gltf_quat forms it
TC_HD TckQ tck_quat(const float* r) {
    TCK_NO_CONTRACT
    const double r0 = (double)r[0], r1 = (double)r[1], r2 = (double)r[2];
    const double theta = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
    const double k = tck_half_sinc(theta);
    return tck_q(cos(theta / 2.0), k * r0, k * r1, k * r2);
}
TC_HD TckQ tck_mul(TckQ a, TckQ b) {
    TCK_NO_CONTRACT
    return tck_q(((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z, ((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y,
                 ((a.w * b.y - a.x * b.z) + a.y * b.w) + a.z * b.x, ((a.w * b.z + a.x * b.y) - a.y * b.x) + a.z * b.w);
}
TC_HD TckQ tck_conj(TckQ q) { return tck_q(q.w, -q.x, -q.y, -q.z); }
// R . v = v + w t + u x t with u = (x, y, z), t = 2 (u x v)
TC_HD TckV tck_rot(TckQ q, TckV v) {
    TCK_NO_CONTRACT
    const TckV u = tck_v(q.x, q.y, q.z);
    const TckV t = tck_scale(tck_cross(u, v), 2.0);
    return tck_add(tck_add(v, tck_scale(t, q.w)), tck_cross(u, t));
}
// the rotation about the unit axis n by the angle phi
TC_HD TckQ tck_about(TckV n, double phi) {
    TCK_NO_CONTRACT
    const double s = sin(phi / 2.0);
    return tck_q(cos(phi / 2.0), n.x * s, n.y * s, n.z * s);
}
// unit quaternion -> rotation vector: w >= 0 first, theta = 2 atan2(|xyz|, w), xyz / half_sinc(theta)
TC_HD TckV tck_rotvec(TckQ q) {
    TCK_NO_CONTRACT
    if (q.w < 0.0) q = tck_q(-q.w, -q.x, -q.y, -q.z);
    const TckV u = tck_v(q.x, q.y, q.z);
    const double theta = 2.0 * atan2(tck_norm(u), q.w);
    return tck_over(u, tck_half_sinc(theta));
}

// ---- step 1: the chain down one leg -------------------------------------------------------------------------------------------------
struct TckLeg { TckV Ph, Pk, Pa, Pe; TckQ Rh, Rk, Ra; };

// R0, P0: the pelvis; qh, qk, qa: the three local rotation vectors; off: the leg's four offsets (hip, knee, ankle, toe), 12 floats
TC_HD TckLeg tck_leg_fk(TckQ R0, TckV P0, const float* qh, const float* qk, const float* qa, const float* off) {
    TckLeg g;
    g.Ph = tck_add(P0, tck_rot(R0, tck_v((double)off[0], (double)off[1], (double)off[2])));
    g.Rh = tck_mul(R0, tck_quat(qh));
    g.Pk = tck_add(g.Ph, tck_rot(g.Rh, tck_v((double)off[3], (double)off[4], (double)off[5])));
    g.Rk = tck_mul(g.Rh, tck_quat(qk));
    g.Pa = tck_add(g.Pk, tck_rot(g.Rk, tck_v((double)off[6], (double)off[7], (double)off[8])));
    g.Ra = tck_mul(g.Rk, tck_quat(qa));
    g.Pe = tck_add(g.Pa, tck_rot(g.Ra, tck_v((double)off[9], (double)off[10], (double)off[11])));
    return g;
}
TC_HD double tck_bone(const float* off) {
    return tck_norm(tck_v((double)off[0], (double)off[1], (double)off[2]));
}

// ---- step 3: the shift of a frame outside the runs --------------------------------------------------------------------------------------
// t0 / t1: the nearest planted frame before / after t, -1 when absent; d0 / d1: their shifts (ignored when absent)
TC_HD TckV tck_ease(int t, int t0, int t1, TckV d0, TckV d1, int blend) {
    TCK_NO_CONTRACT
    if (t0 >= 0 && t1 >= 0 && (t1 - t0) - 1 <= 2 * blend) {
        const double w0 = (double)(t1 - t), w1 = (double)(t - t0), G = (double)(t1 - t0);
        return tck_v((w0 * d0.x + w1 * d1.x) / G, (w0 * d0.y + w1 * d1.y) / G, (w0 * d0.z + w1 * d1.z) / G);
    }
    const double n = (double)(blend + 1);
    const double l0 = t0 >= 0 ? fmax(0.0, 1.0 - (double)(t - t0) / n) : 0.0;
    const double l1 = t1 >= 0 ? fmax(0.0, 1.0 - (double)(t1 - t) / n) : 0.0;
    const TckV a = t0 >= 0 ? tck_scale(d0, l0) : tck_v(0.0, 0.0, 0.0);
    const TckV b = t1 >= 0 ? tck_scale(d1, l1) : tck_v(0.0, 0.0, 0.0);
    return tck_add(a, b);
}

// ---- step 4 -------------------------------------------------------------------------------------------------------------------------------
// the clamped length r' of the wanted hip-to-ankle vector; returns 0: the frame is left as it is (d = 0 or no direction),
// 1: within reach, 2: clamped
TC_HD int tck_reach(TckV H, TckV A, TckV d, double l1, double l2, double reach, double* rp_out) {
    TCK_NO_CONTRACT
    if (tck_is_zero(d)) return 0;
    const double r = tck_norm(tck_sub(A, H));
    const double nv = tck_norm(tck_sub(tck_add(A, d), H));
    if (nv < TCK_TINY) return 0;
    const double rmax = (l1 + l2) * (1.0 - reach), rmin = fabs(l1 - l2) + reach * (l1 + l2);
    const double rp = fmax(fmin(nv, fmax(rmax, r)), rmin);
    *rp_out = rp;
    return rp != nv ? 2 : 1;
}

struct TckSolve { int status; TckV qh, qk, qa; };          // status as tck_reach; the rotation vectors are set when status != 0

TC_HD TckSolve tck_solve(TckQ R0, TckLeg g, TckV d, double l1, double l2, double reach) {
    TCK_NO_CONTRACT
    TckSolve s;
    s.qh = s.qk = s.qa = tck_v(0.0, 0.0, 0.0);
    double rp = 0.0;
    s.status = tck_reach(g.Ph, g.Pa, d, l1, l2, reach, &rp);
    if (s.status == 0) return s;
    const TckV H = g.Ph, K = g.Pk, A = g.Pa;
    const double r = tck_norm(tck_sub(A, H));
    const TckV vp = tck_sub(tck_add(A, d), H);
    const double nv = tck_norm(vp);
    const TckV a = tck_sub(K, H), b = tck_sub(A, K);
    const TckV c = tck_cross(a, b);
    const double nc = tck_norm(c);
    const double theta = atan2(nc, tck_dot(a, b));
    TckV n;
    if (nc < TCK_TINY * l1 * l2) {          // a straight (or folded) leg: the hip's x axis, made perpendicular to the thigh
        const TckV x = tck_rot(g.Rh, tck_v(1.0, 0.0, 0.0));
        const TckV p = tck_sub(x, tck_scale(a, tck_dot(x, a) / tck_dot(a, a)));
        const double np_ = tck_norm(p);
        if (np_ < TCK_TINY) {
            s.status = 0;
            return s;
        }
        n = tck_over(p, np_);
    } else {
        n = tck_over(c, nc);
    }
    const double cs = fmax(-1.0, fmin(1.0, ((l1 * l1 + l2 * l2) - rp * rp) / ((2.0 * l1) * l2)));
    const double delta = rp == r ? 0.0 : (TCK_PI - acos(cs)) - theta;
    const TckQ S1 = tck_about(n, delta);
    const TckV w = tck_sub(tck_add(K, tck_rot(S1, b)), H);          // A1 - H
    const TckV u1 = tck_over(w, tck_norm(w)), u2 = tck_over(vp, nv);
    const TckV cr = tck_cross(u1, u2);
    const double ncr = tck_norm(cr), dt = tck_dot(u1, u2);
    TckQ S2 = tck_q(1.0, 0.0, 0.0, 0.0);
    if (ncr < 1e-300) {
        if (dt < 0.0) {          // antiparallel: no shortest arc
            s.status = 0;
            return s;
        }
    } else {
        S2 = tck_about(tck_over(cr, ncr), atan2(ncr, dt));
    }
    const TckQ Rh2 = tck_mul(S2, g.Rh);
    const TckQ Rk2 = tck_mul(tck_mul(S2, S1), g.Rk);
    s.qh = tck_rotvec(tck_mul(tck_conj(R0), Rh2));
    s.qk = tck_rotvec(tck_mul(tck_conj(Rh2), Rk2));
    s.qa = tck_rotvec(tck_mul(tck_conj(Rk2), g.Ra));
    return s;
}
