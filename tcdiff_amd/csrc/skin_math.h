// The per-pose part of skinning an SMPL body (include/tcdiff_skin.h, launch 1): rotation vectors -> rotation matrices, the pose
// feature, the joints' global transforms along the tree, the twelve floats A_j per joint and the posed joints, as one plain
// function (no HIP builtins), so that the same source compiles
//   * as __device__ code into libtcdiff_gfx950.so (csrc/skin.hip), and
//   * as host code under g++ (tests/host/skin_host.cpp), checked on the CPU against the numpy restatement
//     (tests/test_skin_cpu.py) before it ever runs on a GPU.
// float64 arithmetic on the float32 inputs, contraction off (g++: build with -ffp-contract=off), every sum in the order the header
// writes it, each result rounded to float32 once, at the store.
//
// The series below theta = TC_SKIN_SMALL, t2 = theta^2:
//   sin(theta) / theta         = 1 - t2 / 6 + t2^2 / 120 - ...      evaluated as (1 - t2 / 6) + t2 t2 / 120
//   (1 - cos(theta)) / theta^2 = 1/2 - t2 / 24 + t2^2 / 720 - ...   evaluated as (0.5 - t2 / 24) + t2 t2 / 720
// the first term left out is below 1e-18 / 5040 and 1e-18 / 40320 of the value: nothing in float64.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define TC_SKIN_HD __host__ __device__ __forceinline__
#else
#define TC_SKIN_HD static inline
#endif
#if defined(__clang__)
#define TC_SKIN_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TC_SKIN_NO_CONTRACT
#endif

#define TC_SKIN_JOINTS 24
#define TC_SKIN_FEAT_USED 207             // 9 x 23; the stored row is TC_SKIN_FEAT = 208 floats, the last one zero
#define TC_SKIN_SMALL 1e-3

// r[3] -> R[9], row-major
TC_SKIN_HD void skin_rodrigues(const float* r, double* R) {
    TC_SKIN_NO_CONTRACT
    const double r0 = (double)r[0], r1 = (double)r[1], r2 = (double)r[2];
    const double x00 = r0 * r0, x11 = r1 * r1, x22 = r2 * r2;
    const double theta = sqrt((x00 + x11) + x22);
    const double t2 = theta * theta;
    double a, b;
    if (theta < TC_SKIN_SMALL) {
        a = (1.0 - t2 / 6.0) + t2 * t2 / 120.0;
        b = (0.5 - t2 / 24.0) + t2 * t2 / 720.0;
    } else {                                                            // a NaN theta comes here and stays NaN
        a = sin(theta) / theta;
        b = (1.0 - cos(theta)) / t2;
    }
    const double x01 = r0 * r1, x02 = r0 * r2, x12 = r1 * r2;
    const double a0 = a * r0, a1 = a * r1, a2 = a * r2;
    R[0] = 1.0 - b * (x11 + x22);
    R[1] = b * x01 - a2;
    R[2] = b * x02 + a1;
    R[3] = b * x01 + a2;
    R[4] = 1.0 - b * (x00 + x22);
    R[5] = b * x12 - a0;
    R[6] = b * x02 - a1;
    R[7] = b * x12 + a0;
    R[8] = 1.0 - b * (x00 + x11);
}

// One pose.  r [24][3], trans [3], J [24][3], offsets [24][3] float32; parents [24] (validated: exactly one root, every other
// parent before its child); feat [208], A [24][12] and, unless NULL, joints_out [24][3] are written.  G is the caller's scratch of
// 24 x 12 doubles (registers or private memory on the device).
TC_SKIN_HD void skin_pose(const float* r, const float* trans, const float* J, const float* offsets, const int* parents, int smpl_origin,
                          double* G, float* feat, float* A, float* joints_out) {
    TC_SKIN_NO_CONTRACT
    double s[3];
    int root = 0;
    for (int j = 0; j < TC_SKIN_JOINTS; ++j)
        if (parents[j] < 0 || parents[j] >= TC_SKIN_JOINTS) root = j;
    for (int c = 0; c < 3; ++c) s[c] = smpl_origin ? (double)trans[c] : (double)trans[c] - (double)J[3 * root + c];
    for (int j = 0; j < TC_SKIN_JOINTS; ++j) {
        double R[9];
        skin_rodrigues(r + 3 * j, R);
        if (j > 0)
            for (int e = 0; e < 9; ++e) feat[9 * (j - 1) + e] = (float)(e % 4 == 0 ? R[e] - 1.0 : R[e]);
        double* g = G + 12 * j;
        if (j == root) {
            for (int a = 0; a < 3; ++a) {
                for (int b = 0; b < 3; ++b) g[4 * a + b] = R[3 * a + b];
                g[4 * a + 3] = (double)J[3 * j + a];
            }
        } else {
            const double* p = G + 12 * parents[j];
            const double o0 = (double)offsets[3 * j], o1 = (double)offsets[3 * j + 1], o2 = (double)offsets[3 * j + 2];
            for (int a = 0; a < 3; ++a) {
                for (int b = 0; b < 3; ++b) g[4 * a + b] = (p[4 * a] * R[b] + p[4 * a + 1] * R[3 + b]) + p[4 * a + 2] * R[6 + b];
                g[4 * a + 3] = ((p[4 * a] * o0 + p[4 * a + 1] * o1) + p[4 * a + 2] * o2) + p[4 * a + 3];
            }
        }
        const double j0 = (double)J[3 * j], j1 = (double)J[3 * j + 1], j2 = (double)J[3 * j + 2];
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) A[12 * j + 4 * a + b] = (float)g[4 * a + b];
            A[12 * j + 4 * a + 3] = (float)(g[4 * a + 3] - ((g[4 * a] * j0 + g[4 * a + 1] * j1) + g[4 * a + 2] * j2));
            if (joints_out) joints_out[3 * j + a] = (float)(g[4 * a + 3] + s[a]);
        }
    }
    feat[TC_SKIN_FEAT_USED] = 0.0f;
}

// the shift of a pose as the vertex kernel adds it: float64, rounded once
TC_SKIN_HD float skin_shift(float trans_c, float j_root_c, int smpl_origin) {
    TC_SKIN_NO_CONTRACT
    return smpl_origin ? trans_c : (float)((double)trans_c - (double)j_root_c);
}
