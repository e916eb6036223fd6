// csrc/group_math.h built for the host: a stand-alone program that evaluates the group metrics of one clip with the SAME functions the
// HIP kernels compile, in plain loops, for tests/test_group_cpu.py to compare with the numpy restatement (under -fsanitize=address,
// undefined).  usage: group_host in.bin out.bin
//   in:  int32 dn, T, up, window, max_lag; float64 sigma_floor, radii[24]; int32 parents[24]; float32 joints[dn][T][24][3]
//   out: float64, per pair (a < b, lexicographic): gap[T], closest[T], crossings, sync, sync_lag, sync_zero
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "group_math.h"

static void need(bool ok, const char* what) {
    if (!ok) {
        fprintf(stderr, "group_host: %s\n", what);
        exit(2);
    }
}

// x (24 rows of N) -> z in place and sigma[24], every sum in ascending t
static void standardise(std::vector<double>& x, int N, double* sigma) {
    for (int j = 0; j < TCG_J; ++j) {
        if (N < 1) {
            sigma[j] = NAN;
            continue;
        }
        double* xj = x.data() + (size_t)j * N;
        double sum = 0.0, ss = 0.0;
        for (int t = 0; t < N; ++t) sum = sum + xj[t];
        const double mu = sum / (double)N;
        for (int t = 0; t < N; ++t) {
            const double d = xj[t] - mu;
            ss = ss + d * d;
        }
        sigma[j] = sqrt(ss / (double)N);
        for (int t = 0; t < N; ++t) xj[t] = tcg_standard(xj[t], mu, sigma[j]);
    }
}

int main(int argc, char** argv) {
    need(argc == 3, "usage: group_host in.bin out.bin");
    FILE* f = fopen(argv[1], "rb");
    need(f != NULL, "cannot open the input");
    int head[5], parents[TCG_J];
    double sigma_floor, radii[TCG_J];
    need(fread(head, sizeof(int), 5, f) == 5 && fread(&sigma_floor, sizeof(double), 1, f) == 1 &&
             fread(radii, sizeof(double), TCG_J, f) == TCG_J && fread(parents, sizeof(int), TCG_J, f) == TCG_J,
         "short header");
    const int dn = head[0], T = head[1], up = head[2], window = head[3], max_lag = head[4], N = T - 1;
    need(dn >= 2 && dn <= 64 && T >= 1 && T <= 100000 && up >= 0 && up <= 2 && window >= 0 && max_lag >= 0, "bad sizes");
    for (int j = 1; j < TCG_J; ++j) need(parents[j] >= 0 && parents[j] < j, "bad parents");
    const size_t per = (size_t)T * TCG_J * 3;
    std::vector<float> J((size_t)dn * per);
    need(fread(J.data(), sizeof(float), J.size(), f) == J.size(), "short joints");
    fclose(f);

    std::vector<std::vector<double>> z(dn);
    std::vector<double> sigma((size_t)dn * TCG_J);
    for (int d = 0; d < dn; ++d) {
        z[d].assign((size_t)TCG_J * (N > 0 ? N : 0), 0.0);
        for (int t = 0; t < N; ++t)
            for (int j = 0; j < TCG_J; ++j)
                z[d][(size_t)j * N + t] = tcg_speed(J.data() + d * per + (size_t)t * TCG_J * 3, J.data() + d * per + (size_t)(t + 1) * TCG_J * 3, j);
        standardise(z[d], N > 0 ? N : 0, sigma.data() + (size_t)d * TCG_J);
    }

    std::vector<double> out;
    for (int a = 0; a < dn; ++a)
        for (int b = a + 1; b < dn; ++b) {
            const float* A = J.data() + a * per;
            const float* B = J.data() + b * per;
            std::vector<double> codes;
            for (int t = 0; t < T; ++t) {
                const float* Ja = A + (size_t)t * TCG_J * 3;
                const float* Jb = B + (size_t)t * TCG_J * 3;
                TcgBest best;
                best.v = 0.0;
                best.code = -1;
                for (int k = 0; k < TCG_BONE_PAIRS; ++k) {
                    const int i = 1 + k / 23, j = 1 + k % 23, pi = parents[i], pj = parents[j];
                    const double d = tcg_seg_dist(tcg_v(Ja[3 * pi], Ja[3 * pi + 1], Ja[3 * pi + 2]), tcg_v(Ja[3 * i], Ja[3 * i + 1], Ja[3 * i + 2]),
                                                  tcg_v(Jb[3 * pj], Jb[3 * pj + 1], Jb[3 * pj + 2]), tcg_v(Jb[3 * j], Jb[3 * j + 1], Jb[3 * j + 2]));
                    TcgBest cand;
                    cand.v = tcg_gap(d, radii[i], radii[j]);
                    cand.code = TCG_J * i + j;
                    if (best.code < 0 || tcg_before(cand, best)) best = cand;
                }
                out.push_back(best.v);
                codes.push_back((double)best.code);
            }
            out.insert(out.end(), codes.begin(), codes.end());
            long crossings = 0;
            for (int t = 0; t < N; ++t) {
                double sa[4], sb[4];
                tcg_floor(A + (size_t)t * TCG_J * 3, up, &sa[0], &sa[1]);
                tcg_floor(A + (size_t)(t + 1) * TCG_J * 3, up, &sa[2], &sa[3]);
                const long lo = (long)t - window < 0 ? 0 : (long)t - window, hi = (long)t + window > N - 1 ? N - 1 : (long)t + window;
                for (long s = lo; s <= hi; ++s) {
                    tcg_floor(B + (size_t)s * TCG_J * 3, up, &sb[0], &sb[1]);
                    tcg_floor(B + (size_t)(s + 1) * TCG_J * 3, up, &sb[2], &sb[3]);
                    crossings += tcg_cross(sa, sb);
                }
            }
            out.push_back((double)crossings);
            const int L = tcg_lags(T, max_lag);
            double best = NAN, zero = NAN;
            int best_lag = 0, seen = 0;
            for (int l = -L; L >= 0 && l <= L; ++l) {
                double R = 0.0;
                int n = 0;
                for (int j = 0; j < TCG_J; ++j) {
                    if (!(sigma[(size_t)a * TCG_J + j] > sigma_floor && sigma[(size_t)b * TCG_J + j] > sigma_floor)) continue;
                    double sum = 0.0;
                    for (int t = l < 0 ? -l : 0; t < (l < 0 ? N : N - l); ++t)
                        sum = tcg_corr_add(sum, z[a][(long)j * N + t], z[b][(long)j * N + t + l]);
                    R = R + sum / (double)(N - (l < 0 ? -l : l));
                    ++n;
                }
                if (!n) break;
                R = R / (double)n;
                if (!seen || tcg_better_lag(R, l, best, best_lag)) {
                    best = R;
                    best_lag = l;
                }
                seen = 1;
                if (l == 0) zero = R;
            }
            out.push_back(best);
            out.push_back((double)best_lag);
            out.push_back(zero);
        }
    f = fopen(argv[2], "wb");
    need(f != NULL, "cannot open the output");
    need(fwrite(out.data(), sizeof(double), out.size(), f) == out.size(), "short write");
    fclose(f);
    return 0;
}
