// The relational ("geometric") features of a dance: the 28 points of a frame and the six predicate kinds of
// include/tcdiff_hip_ext.h as plain per-frame functions (no memory traffic of their own, no HIP builtins), so that the same
// source compiles
//   * as __device__ code into libtcdiff_gfx950.so (csrc/geometric.hip), and
//   * as host code under g++ (tests/host/geometric_host.cpp): the decisions are checked on the CPU against the numpy restatement
//     (tests/test_geometric_cpu.py) before they ever run on a GPU.
// float64 arithmetic on the float32 joints, contraction off in every function (g++: build with -ffp-contract=off).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define TC_GEO_HD __host__ __device__ __forceinline__
#else
#define TC_GEO_HD static inline
#endif
#if defined(__clang__)
#define TC_GEO_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TC_GEO_NO_CONTRACT
#endif

#define TC_GEO_JOINTS 24
#define TC_GEO_N_KINDS 6          // TC_GEO_PLANE .. TC_GEO_FAST of the header, in its order
#define TC_GEO_N_POINTS 28        // TC_GEO_POINTS of the header
#define TC_GEO_DEG 57.29577951308232      // 180 / pi

struct GeoRow { int kind, a, b, c, p; double lo, hi; };
struct G3 { double x, y, z; };

// a row the kernel may evaluate: its kind and all four point indices in range, whether or not the kind reads them
TC_GEO_HD int geo_row_valid(int kind, int a, int b, int c, int p) {
    return kind >= 0 && kind < TC_GEO_N_KINDS && a >= 0 && a < TC_GEO_N_POINTS && b >= 0 && b < TC_GEO_N_POINTS && c >= 0 &&
           c < TC_GEO_N_POINTS && p >= 0 && p < TC_GEO_N_POINTS;
}

// the minimum of the 24 joints' `up` component; NaN as soon as one of them is NaN.  F: the frame's [24][3] floats
TC_GEO_HD double geo_floor(const float* F, int up) {
    double m = (double)F[up];
    for (int j = 1; j < TC_GEO_JOINTS; ++j) {
        const double x = (double)F[3 * j + up];
        if (x < m || x != x) m = x;         // (once m is NaN neither test is true again)
    }
    return m;
}

// point i (0 .. 27) of a frame whose floor is fl
TC_GEO_HD G3 geo_point(const float* F, double fl, int up, int i) {
    G3 r;
    if (i < TC_GEO_JOINTS) {
        r.x = (double)F[3 * i];
        r.y = (double)F[3 * i + 1];
        r.z = (double)F[3 * i + 2];
        return r;
    }
    const double v = i == 24 ? 0.0 : (i == 25 ? 1.0 : (i == 26 ? -1.0 : fl));
    r.x = up == 0 ? v : 0.0;
    r.y = up == 1 ? v : 0.0;
    r.z = up == 2 ? v : 0.0;
    return r;
}

TC_GEO_HD G3 geo_sub(G3 a, G3 b) {
    TC_GEO_NO_CONTRACT
    G3 r;
    r.x = a.x - b.x;
    r.y = a.y - b.y;
    r.z = a.z - b.z;
    return r;
}
TC_GEO_HD double geo_dot(G3 a, G3 b) {
    TC_GEO_NO_CONTRACT
    const double xx = a.x * b.x, yy = a.y * b.y, zz = a.z * b.z;
    return (xx + yy) + zz;
}
TC_GEO_HD G3 geo_cross(G3 a, G3 b) {
    TC_GEO_NO_CONTRACT
    G3 r;
    const double yz = a.y * b.z, zy = a.z * b.y, zx = a.z * b.x, xz = a.x * b.z, xy = a.x * b.y, yx = a.y * b.x;
    r.x = yz - zy;
    r.y = zx - xz;
    r.z = xy - yx;
    return r;
}
TC_GEO_HD double geo_norm(G3 a) { return sqrt(geo_dot(a, a)); }
TC_GEO_HD int geo_finite(double v) { return v == v && fabs(v) <= 1.7976931348623157e308; }

// Does the row's predicate hold at a frame?  F, fl: the frame's joints and floor; Fp, flp: those of the frame before; tau: the
// time per frame.  The row must be valid (geo_row_valid).
TC_GEO_HD int geo_holds(const GeoRow& r, const float* F, double fl, const float* Fp, double flp, int up, double tau) {
    TC_GEO_NO_CONTRACT
    double v;
    switch (r.kind) {
        case 0: {   // PLANE: the signed distance of p from the plane through a, b, c
            const G3 a = geo_point(F, fl, up, r.a);
            const G3 n = geo_cross(geo_sub(geo_point(F, fl, up, r.c), a), geo_sub(geo_point(F, fl, up, r.b), a));
            v = geo_dot(n, geo_sub(geo_point(F, fl, up, r.p), a)) / geo_norm(n);
            break;
        }
        case 1: {   // NPLANE: the signed distance of p from the plane through c with normal b - a
            const G3 n = geo_sub(geo_point(F, fl, up, r.b), geo_point(F, fl, up, r.a));
            v = geo_dot(n, geo_sub(geo_point(F, fl, up, r.p), geo_point(F, fl, up, r.c))) / geo_norm(n);
            break;
        }
        case 2:     // MOVE: the velocity of p relative to a, along b - a
        case 3: {   // NMOVE: the same along the normal of the plane through a, b, c
            const G3 a = geo_point(F, fl, up, r.a);
            const G3 w = geo_sub(geo_sub(geo_point(F, fl, up, r.p), a),
                                 geo_sub(geo_point(Fp, flp, up, r.p), geo_point(Fp, flp, up, r.a)));
            const G3 ba = geo_sub(geo_point(F, fl, up, r.b), a);
            const G3 n = r.kind == 2 ? ba : geo_cross(geo_sub(geo_point(F, fl, up, r.c), a), ba);
            v = geo_dot(w, n) / geo_norm(n) / tau;
            break;
        }
        case 4: {   // ANGLE: between b - a and p - c, degrees
            const G3 u = geo_sub(geo_point(F, fl, up, r.b), geo_point(F, fl, up, r.a));
            const G3 w = geo_sub(geo_point(F, fl, up, r.p), geo_point(F, fl, up, r.c));
            const double c = geo_dot(u, w) / (geo_norm(u) * geo_norm(w));
            v = acos(c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c)) * TC_GEO_DEG;        // (a NaN passes the clamp)
            return geo_finite(v) && v > r.lo && v < r.hi;
        }
        default:    // FAST: the speed of p
            v = geo_norm(geo_sub(geo_point(F, fl, up, r.p), geo_point(Fp, flp, up, r.p))) / tau;
            break;
    }
    return geo_finite(v) && v > r.lo;
}
