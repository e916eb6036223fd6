// csrc/skin_math.h built for the host as a stand-alone program (tests/test_skin_cpu.py; g++ -ffp-contract=off):
//   skin_host <in> <out>
// <in>:  int32 P, int32 smpl_origin, int32 parents[24], float32 J[24][3], offsets[24][3], poses[P][24][3], trans[P][3]
// <out>: float32 feat[P][208], A[P][24][12], joints[P][24][3]
#include <cstdio>
#include <vector>

#include "skin_math.h"

static bool read_all(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 3;
    int head[2], parents[TC_SKIN_JOINTS];
    float J[72], offsets[72];
    if (!read_all(in, head, sizeof head) || !read_all(in, parents, sizeof parents) || !read_all(in, J, sizeof J) ||
        !read_all(in, offsets, sizeof offsets) || head[0] < 1)
        return 4;
    const size_t P = (size_t)head[0];
    std::vector<float> poses(P * 72), trans(P * 3), feat(P * 208, 7.0f), A(P * 288, 7.0f), joints(P * 72, 7.0f);
    if (!read_all(in, poses.data(), 4 * poses.size()) || !read_all(in, trans.data(), 4 * trans.size())) return 4;
    fclose(in);
    double G[TC_SKIN_JOINTS * 12];
    for (size_t p = 0; p < P; ++p)
        skin_pose(&poses[p * 72], &trans[p * 3], J, offsets, parents, head[1], G, &feat[p * 208], &A[p * 288], &joints[p * 72]);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 5;
    const bool ok = fwrite(feat.data(), 4, feat.size(), out) == feat.size() && fwrite(A.data(), 4, A.size(), out) == A.size() &&
                    fwrite(joints.data(), 4, joints.size(), out) == joints.size();
    return fclose(out) == 0 && ok ? 0 : 6;
}
