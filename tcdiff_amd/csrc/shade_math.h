// The per-triangle and per-pixel arithmetic of the mesh rasteriser (include/tcdiff_shade.h), shared by csrc/shade.hip and by the
// host build tests/host/shade_host.cpp (g++ -ffp-contract=off), which tests/test_shade_cpu.py holds to the numpy restatement.
// float64 on the fp32 inputs, without contraction, every product, difference and sum in the header's order.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define TC_SHADE_HD __host__ __device__ __forceinline__
#else
#define TC_SHADE_HD static inline
#endif
#if defined(__clang__)
#define TC_SHADE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TC_SHADE_NO_CONTRACT
#endif

// the pixels whose centres lie in a triangle's bounding box, clipped to the image: x0 <= x <= x1, y0 <= y <= y1; empty when
// x0 > x1.  Every value is in 0 .. 32767, so two of them share an int.
struct shade_box {
    int x0, x1, y0, y1;
};

TC_SHADE_HD bool shade_finite(float v) { return fabsf(v) < __builtin_inff(); }

// [lo, hi] (a <= b, both finite) -> the integers n of 0 .. size - 1 with lo <= n + 0.5 <= hi.  The bounds are clamped to the image
// in floating point BEFORE they become integers, so nothing out of range is ever converted; inside the clamp lo - 0.5 is exact.
TC_SHADE_HD void shade_span(float lo, float hi, int size, int* n0, int* n1) {
    const double l = fmax((double)lo, 0.0) - 0.5, h = fmin((double)hi, (double)size) - 0.5;      // l >= -0.5, h <= size - 0.5
    if (!(l <= h) || (double)lo > (double)size || (double)hi < 0.0) {
        *n0 = 1, *n1 = 0;
        return;
    }
    *n0 = (int)ceil(l);                                   // 0 .. size
    *n1 = (int)floor(h);                                  // -1 .. size - 1
    if (*n1 > size - 1) *n1 = size - 1;
    if (*n0 > *n1) *n0 = 1, *n1 = 0;
}

TC_SHADE_HD shade_box shade_make_box(const float* a, const float* b, const float* c, int W, int H) {
    shade_box B;
    B.x0 = B.y0 = 1, B.x1 = B.y1 = 0;
    if (!(shade_finite(a[0]) && shade_finite(a[1]) && shade_finite(a[2]) && shade_finite(b[0]) && shade_finite(b[1]) &&
          shade_finite(b[2]) && shade_finite(c[0]) && shade_finite(c[1]) && shade_finite(c[2])))
        return B;
    shade_span(fminf(a[0], fminf(b[0], c[0])), fmaxf(a[0], fmaxf(b[0], c[0])), W, &B.x0, &B.x1);
    shade_span(fminf(a[1], fminf(b[1], c[1])), fmaxf(a[1], fmaxf(b[1], c[1])), H, &B.y0, &B.y1);
    if (B.x0 > B.x1 || B.y0 > B.y1) B.x0 = B.y0 = 1, B.x1 = B.y1 = 0;
    return B;
}

// a triangle as the pixels read it: each edge's start point and direction, the depths
struct shade_tri {
    double px[3], py[3], dx[3], dy[3];                    // edge i: (a b), (b c), (c a)
    double z[3];                                          // a.z, b.z, c.z
};

TC_SHADE_HD shade_tri shade_setup(const float* a, const float* b, const float* c) {
    TC_SHADE_NO_CONTRACT
    shade_tri t;
    const float* v[4] = {a, b, c, a};
    for (int i = 0; i < 3; ++i) {
        t.px[i] = v[i][0], t.py[i] = v[i][1];
        t.dx[i] = (double)v[i + 1][0] - (double)v[i][0];
        t.dy[i] = (double)v[i + 1][1] - (double)v[i][1];
        t.z[i] = v[i][2];
    }
    return t;
}

// E_i at (px, py); returns whether the triangle covers the point (the box test is the caller's)
TC_SHADE_HD bool shade_edges(const shade_tri& t, double px, double py, double* E, double* area) {
    TC_SHADE_NO_CONTRACT
    for (int i = 0; i < 3; ++i) E[i] = t.dx[i] * (py - t.py[i]) - t.dy[i] * (px - t.px[i]);
    *area = (E[0] + E[1]) + E[2];
    const bool pos = E[0] >= 0.0 && E[1] >= 0.0 && E[2] >= 0.0, neg = E[0] <= 0.0 && E[1] <= 0.0 && E[2] <= 0.0;
    return *area != 0.0 && (pos || neg);
}

TC_SHADE_HD double shade_depth(const shade_tri& t, const double* E, double area) {
    TC_SHADE_NO_CONTRACT
    return ((E[1] * t.z[0] + E[2] * t.z[1]) + E[0] * t.z[2]) / area;
}

// the Lambert factor k from the three vertex normals, the edge functions and the light
TC_SHADE_HD double shade_factor(const float* na, const float* nb, const float* nc, const double* E, const float* light, double ambient) {
    TC_SHADE_NO_CONTRACT
    double n[3];
    for (int k = 0; k < 3; ++k) n[k] = (E[1] * (double)na[k] + E[2] * (double)nb[k]) + E[0] * (double)nc[k];
    const double dot = (n[0] * (double)light[0] + n[1] * (double)light[1]) + n[2] * (double)light[2];
    const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    if (len == 0.0) return ambient;
    const double k = ambient + (1.0 - ambient) * (fabs(dot) / len);
    return k == k ? k : ambient;
}

TC_SHADE_HD unsigned char shade_level(unsigned char colour, double k) {
    TC_SHADE_NO_CONTRACT
    const double v = floor((double)colour * k + 0.5);
    return (unsigned char)(v > 255.0 ? 255.0 : (v < 0.0 ? 0.0 : v));
}
