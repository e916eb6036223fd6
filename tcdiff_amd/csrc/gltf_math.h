// The quaternion of a glTF rotation key frame (include/tcdiff_gltf.h): rotation vector -> (x, y, z, w), the root's turn to Y-up,
// and the test that flips a channel's sign, as plain functions (no memory traffic of their own, no HIP builtins), so that the same
// source compiles
//   * as __device__ code into libtcdiff_gfx950.so (csrc/gltf.hip), and
//   * as host code under g++ (tests/host/gltf_host.cpp), checked on the CPU against the numpy restatement
//     (tests/test_gltf_cpu.py) before it ever runs on a GPU.
// float64 arithmetic on the float32 inputs, contraction off in every function (g++: build with -ffp-contract=off).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define TC_GLTF_HD __host__ __device__ __forceinline__
#else
#define TC_GLTF_HD static inline
#endif
#if defined(__clang__)
#define TC_GLTF_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TC_GLTF_NO_CONTRACT
#endif

#define TC_GLTF_JOINTS 24
#define TC_GLTF_PER_DANCER 99             // floats per frame and dancer: 3 of trans, 24 x 4 of rot
#define TC_GLTF_SMALL 1e-3                // below it the series of sin(theta / 2) / theta
#define TC_GLTF_FW 0.70710678118654757    // sqrt(1/2): f = (-FW, 0, 0, FW), the turn by -90 degrees about x

struct GltfQ { double x, y, z, w; };

// r[3] -> the quaternion of the header; root: f (x) q on the left
TC_GLTF_HD GltfQ gltf_quat(const float* r, int root) {
    TC_GLTF_NO_CONTRACT
    const double r0 = (double)r[0], r1 = (double)r[1], r2 = (double)r[2];
    const double theta = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
    const double a2 = theta * theta;
    const double k = theta < TC_GLTF_SMALL ? (0.5 - a2 / 48.0) + a2 * a2 / 3840.0 : sin(theta / 2.0) / theta;
    GltfQ q;
    q.x = k * r0;
    q.y = k * r1;
    q.z = k * r2;
    q.w = cos(theta / 2.0);
    if (root) {
        const double fw = TC_GLTF_FW, fx = -TC_GLTF_FW;
        GltfQ p;
        p.x = fw * q.x + fx * q.w;
        p.y = fw * q.y - fx * q.z;
        p.z = fw * q.z + fx * q.y;
        p.w = fw * q.w - fx * q.x;
        return p;
    }
    return q;
}

// does the sign change between q_(t-1) = a and q_t = b?  A zero or NaN dot product does not flip.
TC_GLTF_HD int gltf_flips(const GltfQ a, const GltfQ b) {
    TC_GLTF_NO_CONTRACT
    return ((b.x * a.x + b.y * a.y) + b.z * a.z) + b.w * a.w < 0.0;
}
