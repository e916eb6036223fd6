// The predicates of mesh-level contact (include/tcdiff_meshcontact.h): is an edge crossed, does a face cover a point and with which
// sign, how far is a point from a triangle, and the orders of the maxima -- plain functions (no memory traffic of their own, no HIP
// builtins), so that the same source compiles
//   * as __device__ code into libtcdiff_gfx950.so (csrc/meshcontact.hip), and
//   * as host code under g++ (tests/host/meshcontact_host.cpp), checked on the CPU against the numpy restatement
//     (tests/test_meshcontact_cpu.py) before it ever runs on a GPU.
// float64 arithmetic on the float32 inputs, contraction off in every function (g++: build with -ffp-contract=off).  A point or a
// vertex is three doubles (x, y, z) in the header's sense: already permuted by `up`.
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
#define TCM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TCM_NO_CONTRACT
#endif

#define TCM_SWAP01 1                      // i0 > i1: the edge {i0, i1} is evaluated from i1
#define TCM_SWAP12 2
#define TCM_SWAP20 4

// where the components x, y, z of the header sit in a stored vertex
TC_HD int tcm_axis_x(int up) { return up == 0 ? 1 : 0; }
TC_HD int tcm_axis_y(int up) { return up == 2 ? 1 : 2; }

// the order flags of a face
TC_HD int tcm_flags(int i0, int i1, int i2) { return (i0 > i1 ? TCM_SWAP01 : 0) | (i1 > i2 ? TCM_SWAP12 : 0) | (i2 > i0 ? TCM_SWAP20 : 0); }

// step 2: is the edge u -> w (u the vertex of the lower index) crossed by the ray from (px, py) in +x?
TC_HD int tcm_crossed(double px, double py, double ux, double uy, double wx, double wy) {
    TCM_NO_CONTRACT
    if ((uy > py) == (wy > py)) return 0;
    const double xe = ux + ((py - uy) / (wy - uy)) * (wx - ux);
    return px < xe;
}

// steps 3 to 5: what the face A, B, C (nine doubles) adds to w(p): 0 if it does not cover p, has D == 0 or z_hit <= p.z; where it adds,
// gap = z_hit - p.z (the face lies that far above p: an upper bound of p's distance to the surface) and area = D
TC_HD int tcm_wind_gap(const double* p, const double* A, const double* B, const double* C, int flags, double* gap, double* area) {
    TCM_NO_CONTRACT
    const int c01 = (flags & TCM_SWAP01) ? tcm_crossed(p[0], p[1], B[0], B[1], A[0], A[1]) : tcm_crossed(p[0], p[1], A[0], A[1], B[0], B[1]);
    const int c12 = (flags & TCM_SWAP12) ? tcm_crossed(p[0], p[1], C[0], C[1], B[0], B[1]) : tcm_crossed(p[0], p[1], B[0], B[1], C[0], C[1]);
    const int c20 = (flags & TCM_SWAP20) ? tcm_crossed(p[0], p[1], A[0], A[1], C[0], C[1]) : tcm_crossed(p[0], p[1], C[0], C[1], A[0], A[1]);
    if (!((c01 + c12 + c20) & 1)) return 0;
    const double bx = B[0] - A[0], by = B[1] - A[1], cx = C[0] - A[0], cy = C[1] - A[1], qx = p[0] - A[0], qy = p[1] - A[1];
    const double D = bx * cy - by * cx;
    if (D == 0.0) return 0;
    const double l1 = (qx * cy - qy * cx) / D;
    const double l2 = (bx * qy - by * qx) / D;
    const double z_hit = (A[2] + l1 * (B[2] - A[2])) + l2 * (C[2] - A[2]);
    if (!(z_hit > p[2])) return 0;
    *gap = z_hit - p[2];
    *area = D;
    return D > 0.0 ? 1 : -1;
}
TC_HD int tcm_wind(const double* p, const double* A, const double* B, const double* C, int flags) {
    double gap, area;
    return tcm_wind_gap(p, A, B, C, flags, &gap, &area);
}

TC_HD double tcm_dot(const double* a, const double* b) { TCM_NO_CONTRACT return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// step 6: the squared distance from p to the triangle A, B, C; the distance is its square root, and as the correctly rounded root is
// monotone, the root of the smallest square is the smallest distance to the bit
TC_HD double tcm_tri_dist2(const double* p, const double* A, const double* B, const double* C) {
    TCM_NO_CONTRACT
    double ab[3], ac[3], ap[3], bp[3], cp[3], q[3], e[3];
    for (int k = 0; k < 3; ++k) {
        ab[k] = B[k] - A[k];
        ac[k] = C[k] - A[k];
        ap[k] = p[k] - A[k];
        bp[k] = p[k] - B[k];
        cp[k] = p[k] - C[k];
    }
    const double d1 = tcm_dot(ab, ap), d2 = tcm_dot(ac, ap), d3 = tcm_dot(ab, bp), d4 = tcm_dot(ac, bp), d5 = tcm_dot(ab, cp), d6 = tcm_dot(ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4, g = d4 - d3, h = d5 - d6;
    if (d1 <= 0.0 && d2 <= 0.0) {
        for (int k = 0; k < 3; ++k) q[k] = A[k];
    } else if (d3 >= 0.0 && d4 <= d3) {
        for (int k = 0; k < 3; ++k) q[k] = B[k];
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double s = d1 / (d1 - d3);
        for (int k = 0; k < 3; ++k) q[k] = A[k] + s * ab[k];
    } else if (d6 >= 0.0 && d5 <= d6) {
        for (int k = 0; k < 3; ++k) q[k] = C[k];
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double s = d2 / (d2 - d6);
        for (int k = 0; k < 3; ++k) q[k] = A[k] + s * ac[k];
    } else if (va <= 0.0 && g >= 0.0 && h >= 0.0) {
        const double s = g / (g + h);
        for (int k = 0; k < 3; ++k) q[k] = B[k] + s * (C[k] - B[k]);
    } else {
        const double s = (va + vb) + vc, v = vb / s, w = vc / s;
        for (int k = 0; k < 3; ++k) q[k] = (A[k] + v * ab[k]) + w * ac[k];
    }
    for (int k = 0; k < 3; ++k) e[k] = p[k] - q[k];
    return tcm_dot(e, e);
}
TC_HD double tcm_tri_dist(const double* p, const double* A, const double* B, const double* C) { return sqrt(tcm_tri_dist2(p, A, B, C)); }

// the broad phase of step 6, in float32 with room for its rounding.  An inside vertex has a counted face `gap` above it, so its depth
// is at most gap; a face whose box is further from p than a known upper bound of the depth cannot attain the minimum.
// tcm_bound2: an upper bound (squared, 1 % and 3e-5 m of slack) from a gap or a distance already found; tcm_box_dist2: a lower bound
// (squared, 1 % of slack) of the distance from p to the triangle f[9].  Skip the face iff tcm_box_dist2 > bound.
#define TCM_MIN_AREA 1e-10                // a counted face with |D| below it gives no bound: its z_hit may be rounding
TC_HD float tcm_bound2(float d) { return d * d * 1.01f + 1e-9f; }
TC_HD float tcm_fmin(float a, float b) { return a < b ? a : b; }
TC_HD float tcm_fmax(float a, float b) { return a > b ? a : b; }
TC_HD float tcm_box_dist2(const float* p, const float* f) {
    float s = 0.0f;
    for (int k = 0; k < 3; ++k) {
        const float lo = tcm_fmin(tcm_fmin(f[k], f[3 + k]), f[6 + k]), hi = tcm_fmax(tcm_fmax(f[k], f[3 + k]), f[6 + k]);
        const float d = tcm_fmax(tcm_fmax(lo - p[k], p[k] - hi), 0.0f);
        s += d * d;
    }
    return s * 0.99f;
}

// the order of the deepest vertex: the larger depth, then the lower key (key < 0: none yet)
TC_HD int tcm_deeper(double da, long ka, double db, long kb) {
    if (ka < 0 || kb < 0) return kb < 0 && ka >= 0;
    return da > db || (da == db && ka < kb);
}

TC_HD int tcm_finite32(float v) { return v - v == 0.0f; }
