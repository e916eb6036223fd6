// Host build (g++ -ffp-contract=off) of tcdiff_amd/csrc/gltf_math.h: the quaternion and the flip test the HIP kernel of
// csrc/gltf.hip calls, with the sign rule of include/tcdiff_gltf.h as a sequential loop, exported for tests/test_gltf_cpu.py
// (compared there with the numpy restatement).
#include "gltf_math.h"

extern "C" {
// smpl_poses [clips][T][dn][24][3], smpl_trans [clips][T][dn][3] -> out [clips][T (1 + 99 dn)]
void host_gltf_block(const float* poses, const float* trans, int clips, int T, int dn, double fps, float* out) {
    const long F = (long)T * (1 + TC_GLTF_PER_DANCER * (long)dn);
    for (long c = 0; c < clips; ++c) {
        float* clip = out + c * F;
        for (int t = 0; t < T; ++t) clip[t] = (float)((double)t / fps);
        for (int d = 0; d < dn; ++d) {
            float* dancer = clip + T + (long)d * TC_GLTF_PER_DANCER * T;
            for (int t = 0; t < T; ++t) {
                const float* p = trans + ((c * T + t) * dn + d) * 3;
                dancer[3L * t] = p[0];
                dancer[3L * t + 1] = p[2];
                dancer[3L * t + 2] = -p[1];
            }
            for (int j = 0; j < TC_GLTF_JOINTS; ++j) {
                float* o = dancer + 3L * T + 4L * j * T;
                GltfQ prev = {0.0, 0.0, 0.0, 1.0};
                double s = 1.0;
                for (int t = 0; t < T; ++t) {
                    const GltfQ q = gltf_quat(poses + (((c * T + t) * dn + d) * TC_GLTF_JOINTS + j) * 3, j == 0);
                    if (t == 0 ? q.w < 0.0 : gltf_flips(prev, q)) s = -s;
                    o[4L * t] = (float)(s * q.x);
                    o[4L * t + 1] = (float)(s * q.y);
                    o[4L * t + 2] = (float)(s * q.z);
                    o[4L * t + 3] = (float)(s * q.w);
                    prev = q;
                }
            }
        }
    }
}

// the flip test on two quaternions given as (x, y, z, w): inputs the rotation vectors cannot reach (a dot product of exactly 0)
int host_gltf_flips(const double* a, const double* b) {
    const GltfQ qa = {a[0], a[1], a[2], a[3]}, qb = {b[0], b[1], b[2], b[3]};
    return gltf_flips(qa, qb);
}
}
