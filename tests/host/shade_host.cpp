// csrc/shade_math.h built for the host as a stand-alone program (tests/test_shade_cpu.py; g++ -ffp-contract=off): one frame of
// the picture of include/tcdiff_shade.h, every triangle at every pixel of its box, no tiles and no chunks.
//   shade_host <in> <out>
// <in>:  int32 dn, V, F, W, H, n_colors, has_under; float32 ambient, light[3]; uint8 background[3], pad;
//        float32 screen[dn][V][3], normals[dn][V][3]; int32 faces[F][3]; uint8 colors[n_colors][3]; uint8 under[H][W][3] if has_under
// <out>: uint8 frame[H][W][3]
#include <cstdio>
#include <vector>

#include "shade_math.h"

static bool read_all(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 3;
    int head[7];
    float shade[4];
    unsigned char bg[4];
    if (!read_all(in, head, sizeof head) || !read_all(in, shade, sizeof shade) || !read_all(in, bg, sizeof bg)) return 4;
    const int dn = head[0], V = head[1], F = head[2], W = head[3], H = head[4], n_colors = head[5], has_under = head[6];
    if (dn < 1 || V < 1 || F < 1 || W < 1 || H < 1 || n_colors < 1) return 4;
    std::vector<float> screen((size_t)dn * V * 3), normals((size_t)dn * V * 3);
    std::vector<int> faces((size_t)F * 3);
    std::vector<unsigned char> colors((size_t)n_colors * 3), under(has_under ? (size_t)H * W * 3 : 0), frame((size_t)H * W * 3);
    if (!read_all(in, screen.data(), 4 * screen.size()) || !read_all(in, normals.data(), 4 * normals.size()) ||
        !read_all(in, faces.data(), 4 * faces.size()) || !read_all(in, colors.data(), colors.size()) ||
        !read_all(in, under.data(), under.size()))
        return 4;
    fclose(in);
    std::vector<double> best_z((size_t)H * W, 0.0);
    std::vector<int> best_g((size_t)H * W, -1);
    std::vector<double> weight((size_t)H * W * 3, 0.0);
    for (int g = 0; g < dn * F; ++g) {
        const int d = g / F, f = g - d * F;
        const int* idx = &faces[(size_t)f * 3];
        if (idx[0] < 0 || idx[0] >= V || idx[1] < 0 || idx[1] >= V || idx[2] < 0 || idx[2] >= V) continue;
        const float* S = &screen[(size_t)d * V * 3];
        const shade_box B = shade_make_box(S + 3 * idx[0], S + 3 * idx[1], S + 3 * idx[2], W, H);
        if (B.x0 > B.x1) continue;
        const shade_tri tri = shade_setup(S + 3 * idx[0], S + 3 * idx[1], S + 3 * idx[2]);
        for (int y = B.y0; y <= B.y1; ++y)
            for (int x = B.x0; x <= B.x1; ++x) {
                double E[3], area;
                if (!shade_edges(tri, x + 0.5, y + 0.5, E, &area)) continue;
                const double z = shade_depth(tri, E, area);
                const size_t i = (size_t)y * W + x;
                if (best_g[i] < 0 || z < best_z[i] || (z == best_z[i] && g < best_g[i])) {
                    best_z[i] = z, best_g[i] = g;
                    weight[3 * i] = E[0], weight[3 * i + 1] = E[1], weight[3 * i + 2] = E[2];
                }
            }
    }
    for (size_t i = 0; i < (size_t)H * W; ++i) {
        unsigned char* o = &frame[3 * i];
        if (best_g[i] < 0) {
            for (int c = 0; c < 3; ++c) o[c] = has_under ? under[3 * i + c] : bg[c];
            continue;
        }
        const int d = best_g[i] / F, f = best_g[i] - d * F;
        const int* idx = &faces[(size_t)f * 3];
        const float* N = &normals[(size_t)d * V * 3];
        const double k = shade_factor(N + 3 * idx[0], N + 3 * idx[1], N + 3 * idx[2], &weight[3 * i], shade + 1, (double)shade[0]);
        for (int c = 0; c < 3; ++c) o[c] = shade_level(colors[3 * (d % n_colors) + c], k);
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 5;
    const bool ok = fwrite(frame.data(), 1, frame.size(), out) == frame.size();
    return fclose(out) == 0 && ok ? 0 : 6;
}
