// csrc/apart_math.h built for the host: a stand-alone program that keeps the dancers of one clip apart with the SAME functions the HIP
// kernels compile, in plain loops, for tests/test_apart_cpu.py to compare with the numpy restatement (under -fsanitize=address,
// undefined).  usage: apart_host in.bin out.bin
//   in:  int32 dn, T, up, iterations, rounds, blend; float64 margin, max_push, radii[24], mobility[dn]; int32 parents[24];
//        float32 pos[T][dn][3], joints[dn][T][24][3]
//   out: float64 shift[dn][T][2], then per pair (a < b, lexicographic) before[T], after[T], flags[T];
//        then float32 pos_out[T][dn][3], joints_out[dn][T][24][3]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "apart_math.h"

static void need(bool ok, const char* what) {
    if (!ok) {
        fprintf(stderr, "apart_host: %s\n", what);
        exit(2);
    }
}

int main(int argc, char** argv) {
    need(argc == 3, "usage: apart_host in.bin out.bin");
    FILE* f = fopen(argv[1], "rb");
    need(f != NULL, "cannot open the input");
    int head[6], parents[TCG_J];
    double scal[2], radii[TCG_J];
    need(fread(head, sizeof(int), 6, f) == 6 && fread(scal, sizeof(double), 2, f) == 2 && fread(radii, sizeof(double), TCG_J, f) == TCG_J,
         "short header");
    const int dn = head[0], T = head[1], up = head[2], iterations = head[3], rounds = head[4], blend = head[5];
    const double margin = scal[0], max_push = scal[1];
    need(dn >= 2 && dn <= 32 && T >= 1 && T <= 100000 && up >= 0 && up <= 2 && iterations >= 0 && rounds >= 0 && blend >= 0, "bad sizes");
    std::vector<double> mob(dn);
    need(fread(mob.data(), sizeof(double), dn, f) == (size_t)dn && fread(parents, sizeof(int), TCG_J, f) == TCG_J, "short tables");
    for (int j = 1; j < TCG_J; ++j) need(parents[j] >= 0 && parents[j] < j, "bad parents");
    parents[0] = 0;
    const size_t per = (size_t)T * TCG_J * 3, P = (size_t)dn * (dn - 1) / 2;
    std::vector<float> pos((size_t)T * dn * 3), J((size_t)dn * per);
    need(fread(pos.data(), sizeof(float), pos.size(), f) == pos.size() && fread(J.data(), sizeof(float), J.size(), f) == J.size(), "short data");
    fclose(f);

    std::vector<double> S((size_t)dn * T * 2, 0.0), m(P * T), u(P * T * 2), before(P * T), after(P * T), flags(P * T, 0.0);
    std::vector<float> pos_out(pos), J_out(J);

    // step 1 for one (pair, frame) of the joints `src` with the shift `shift` (or none): returns the entry gap
    auto demand = [&](const std::vector<float>& src, const double* shift, int a, int b, int t, int its, double* m_out, TcpDir* u_out, int* capped) {
        double Ja[TCG_J * 3], Jb[TCG_J * 3];
        for (int k = 0; k < TCG_J * 3; ++k) {
            const double* sa = shift ? shift + ((size_t)a * T + t) * 2 : NULL;
            const double* sb = shift ? shift + ((size_t)b * T + t) * 2 : NULL;
            Ja[k] = tcp_stage(src[a * per + (size_t)t * TCG_J * 3 + k], k % 3, up, sa ? sa[0] : 0.0, sa ? sa[1] : 0.0);
            Jb[k] = tcp_stage(src[b * per + (size_t)t * TCG_J * 3 + k], k % 3, up, sb ? sb[0] : 0.0, sb ? sb[1] : 0.0);
        }
        const TcpDir dir = tcp_direction(tcp_floor(tcp_joint(Ja, 0), up), tcp_floor(tcp_joint(Jb, 0), up));
        double wa, wb, mm = 0.0, g0 = 0.0;
        const int evaluations = tcp_shares(mob[a], mob[b], &wa, &wb) ? its : 0;
        *capped = 0;
        for (int it = 0;; ++it) {
            const TcgBest best = tcp_gap_range(Ja, Jb, tcp_move(wa, mm, dir, up), tcp_move(wb, mm, dir, up), parents, radii, 0, 1);
            if (it == 0) g0 = best.v;
            if (it >= evaluations) break;
            const int go = tcp_step(best.v, margin, max_push, &mm);
            *capped = go == 2;
            if (go != 1 || it + 1 >= evaluations) break;
        }
        *m_out = mm;
        *u_out = dir;
        return g0;
    };

    for (int r = 0; r < rounds; ++r) {
        size_t p = 0;
        for (int a = 0; a < dn; ++a)
            for (int b = a + 1; b < dn; ++b, ++p)
                for (int t = 0; t < T; ++t) {
                    TcpDir dir;
                    int capped;
                    const double g0 = demand(J, r ? S.data() : NULL, a, b, t, iterations, &m[p * T + t], &dir, &capped);
                    if (r == 0) before[p * T + t] = g0;
                    u[(p * T + t) * 2] = dir.x;
                    u[(p * T + t) * 2 + 1] = dir.y;
                    const int now = (m[p * T + t] > 0.0 ? 1 : 0) | (capped ? 2 : 0);
                    flags[p * T + t] = (double)((int)flags[p * T + t] | now);
                }
        for (int d = 0; d < dn; ++d)
            for (int t = 0; t < T; ++t) {
                TcpDir s;
                s.x = S[((size_t)d * T + t) * 2];
                s.y = S[((size_t)d * T + t) * 2 + 1];
                const int lo = t - blend < 0 ? 0 : t - blend, hi = t > T - 1 - blend ? T - 1 : t + blend;
                for (int x = 0; x < dn; ++x) {
                    if (x == d) continue;
                    const int a = x < d ? x : d, b = x < d ? d : x;
                    double wa, wb;
                    if (!tcp_shares(mob[a], mob[b], &wa, &wb)) continue;
                    const size_t row = ((size_t)a * (2 * dn - a - 1) / 2 + (b - a - 1)) * T;
                    double e = 0.0;
                    for (int k = lo; k <= hi; ++k) {
                        const double cand = tcp_tent(m[row + k], k < t ? t - k : k - t, blend);
                        e = cand > e ? cand : e;
                    }
                    TcpDir dir;
                    dir.x = u[(row + t) * 2];
                    dir.y = u[(row + t) * 2 + 1];
                    s = d == a ? tcp_shift(s, wa, e, dir, -1) : tcp_shift(s, wb, e, dir, +1);
                }
                S[((size_t)d * T + t) * 2] = s.x;
                S[((size_t)d * T + t) * 2 + 1] = s.y;
            }
    }
    const int f0 = up == 0 ? 1 : 0, f1 = up == 2 ? 1 : 2;
    for (int d = 0; d < dn; ++d)
        for (int t = 0; t < T; ++t) {
            const double sx = S[((size_t)d * T + t) * 2], sy = S[((size_t)d * T + t) * 2 + 1];
            if (sx == 0.0 && sy == 0.0) continue;             // the copies made above stand
            for (int r = 0; r < TCG_J + 1; ++r) {
                const bool joint = r < TCG_J;
                const float* src = joint ? &J[d * per + ((size_t)t * TCG_J + r) * 3] : &pos[((size_t)t * dn + d) * 3];
                float* dst = joint ? &J_out[d * per + ((size_t)t * TCG_J + r) * 3] : &pos_out[((size_t)t * dn + d) * 3];
                dst[f0] = tcp_out(src[f0], sx);
                dst[f1] = tcp_out(src[f1], sy);
            }
        }
    size_t p = 0;
    for (int a = 0; a < dn; ++a)
        for (int b = a + 1; b < dn; ++b, ++p)
            for (int t = 0; t < T; ++t) {
                double mm;
                TcpDir dir;
                int capped;
                after[p * T + t] = demand(J_out, NULL, a, b, t, 0, &mm, &dir, &capped);
                if (rounds == 0) before[p * T + t] = after[p * T + t];
            }

    f = fopen(argv[2], "wb");
    need(f != NULL, "cannot open the output");
    need(fwrite(S.data(), sizeof(double), S.size(), f) == S.size(), "short write");
    for (p = 0; p < P; ++p)
        need(fwrite(&before[p * T], sizeof(double), T, f) == (size_t)T && fwrite(&after[p * T], sizeof(double), T, f) == (size_t)T &&
                 fwrite(&flags[p * T], sizeof(double), T, f) == (size_t)T,
             "short write");
    need(fwrite(pos_out.data(), sizeof(float), pos_out.size(), f) == pos_out.size() &&
             fwrite(J_out.data(), sizeof(float), J_out.size(), f) == J_out.size(),
         "short write");
    fclose(f);
    return 0;
}
