// csrc/meshcontact_math.h built for the host: a stand-alone program that evaluates the mesh contact of one clip with the SAME
// functions the HIP kernels compile, in plain loops (every vertex against every face, no boxes, no tiles), for
// tests/test_meshcontact_cpu.py to compare with the numpy restatement (under -fsanitize=address,undefined).
// usage: meshcontact_host in.bin out.bin
//   in:  int32 dn, T, V, F, up; int32 faces[F][3]; float32 vertices[T dn][V][3]
//   out: float64, per pair (a < b, lexicographic) and frame: inside a in b, inside b in a, depth, the deepest vertex's dancer and index
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "meshcontact_math.h"

static void need(bool ok, const char* what) {
    if (!ok) {
        fprintf(stderr, "meshcontact_host: %s\n", what);
        exit(2);
    }
}

static void point(const float* X, int v, int up, double* p) {
    p[0] = (double)X[3 * (size_t)v + tcm_axis_x(up)];
    p[1] = (double)X[3 * (size_t)v + tcm_axis_y(up)];
    p[2] = (double)X[3 * (size_t)v + up];
}

int main(int argc, char** argv) {
    need(argc == 3, "usage: meshcontact_host in.bin out.bin");
    FILE* f = fopen(argv[1], "rb");
    need(f != NULL, "cannot open the input");
    int head[5];
    need(fread(head, sizeof(int), 5, f) == 5, "short header");
    const int dn = head[0], T = head[1], V = head[2], F = head[3], up = head[4];
    need(dn >= 2 && dn <= 64 && T >= 1 && T <= 100000 && V >= 1 && V <= 1000000 && F >= 1 && F <= 1000000 && up >= 0 && up <= 2, "bad sizes");
    std::vector<int> faces((size_t)F * 3);
    need(fread(faces.data(), sizeof(int), faces.size(), f) == faces.size(), "short faces");
    for (int i : faces) need(i >= 0 && i < V, "a face index out of range");
    std::vector<float> X((size_t)T * dn * V * 3);
    need(fread(X.data(), sizeof(float), X.size(), f) == X.size(), "short vertices");
    fclose(f);

    std::vector<double> out;
    long total_skipped = 0, total_faces = 0;
    for (int a = 0; a < dn; ++a)
        for (int b = a + 1; b < dn; ++b)
            for (int t = 0; t < T; ++t) {
                const float* pose[2] = {X.data() + ((size_t)t * dn + a) * V * 3, X.data() + ((size_t)t * dn + b) * V * 3};
                bool valid = true;
                for (int s = 0; s < 2; ++s)
                    for (int k = 0; k < 3 * V; ++k) valid = valid && tcm_finite32(pose[s][k]);
                if (!valid) {
                    const double row[5] = {-1.0, -1.0, NAN, -1.0, -1.0};
                    out.insert(out.end(), row, row + 5);
                    continue;
                }
                double count[2] = {0.0, 0.0}, best = 0.0;
                long key = -1;                                // direction V + vertex
                for (int dir = 0; dir < 2; ++dir) {
                    const float* S = pose[dir];
                    const float* D = pose[1 - dir];
                    for (int v = 0; v < V; ++v) {
                        double p[3], A[3], B[3], C[3];
                        point(S, v, up, p);
                        int w = 0;
                        double above = INFINITY;              // as the kernel keeps it: the nearest counted face above p
                        for (int k = 0; k < F; ++k) {
                            const int i0 = faces[3 * (size_t)k], i1 = faces[3 * (size_t)k + 1], i2 = faces[3 * (size_t)k + 2];
                            point(D, i0, up, A);
                            point(D, i1, up, B);
                            point(D, i2, up, C);
                            double gap, area;
                            const int sign = tcm_wind_gap(p, A, B, C, tcm_flags(i0, i1, i2), &gap, &area);
                            need(sign == tcm_wind(p, A, B, C, tcm_flags(i0, i1, i2)), "tcm_wind and tcm_wind_gap disagree");
                            w += sign;
                            if (sign != 0 && (area >= TCM_MIN_AREA || area <= -TCM_MIN_AREA) && gap < above) above = gap;
                        }
                        if (w == 0) continue;
                        count[dir] += 1.0;
                        double depth = INFINITY;
                        for (int k = 0; k < F; ++k) {
                            point(D, faces[3 * (size_t)k], up, A);
                            point(D, faces[3 * (size_t)k + 1], up, B);
                            point(D, faces[3 * (size_t)k + 2], up, C);
                            const double d = tcm_tri_dist(p, A, B, C);
                            if (d < depth) depth = d;
                        }
                        // the kernel's way: squared distances, faces skipped by their boxes, one root -- the same bits
                        const float pf[3] = {(float)p[0], (float)p[1], (float)p[2]};
                        float bound = tcm_bound2((float)above);
                        double least = INFINITY;
                        long skipped = 0;
                        for (int k = 0; k < F; ++k) {
                            point(D, faces[3 * (size_t)k], up, A);
                            point(D, faces[3 * (size_t)k + 1], up, B);
                            point(D, faces[3 * (size_t)k + 2], up, C);
                            const float ff[9] = {(float)A[0], (float)A[1], (float)A[2], (float)B[0], (float)B[1], (float)B[2],
                                                 (float)C[0], (float)C[1], (float)C[2]};
                            if (tcm_box_dist2(pf, ff) > bound) {
                                ++skipped;
                                continue;
                            }
                            const double d2 = tcm_tri_dist2(p, A, B, C);
                            if (d2 < least) {
                                least = d2;
                                bound = tcm_fmin(bound, (float)d2 * 1.01f + 1e-9f);
                            }
                        }
                        need(sqrt(least) == depth, "skipping faces by their boxes changed a depth");
                        total_skipped += skipped;
                        total_faces += F;
                        if (tcm_deeper(depth, (long)dir * V + v, best, key)) {
                            best = depth;
                            key = (long)dir * V + v;
                        }
                    }
                }
                const double row[5] = {count[0], count[1], best, key < 0 ? -1.0 : (double)(key / V ? b : a), key < 0 ? -1.0 : (double)(key % V)};
                out.insert(out.end(), row, row + 5);
            }
    printf("%ld of %ld faces skipped by their boxes in the distance passes\n", total_skipped, total_faces);
    f = fopen(argv[2], "wb");
    need(f != NULL, "cannot open the output");
    need(fwrite(out.data(), sizeof(double), out.size(), f) == out.size(), "short write");
    fclose(f);
    return 0;
}
