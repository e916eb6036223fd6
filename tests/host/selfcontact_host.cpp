// csrc/selfcontact_math.h and csrc/group_math.h built for the host: a stand-alone program that evaluates the self-contact metric of one
// dancer with the SAME functions the HIP kernels compile, in plain loops, for tests/test_selfcontact_cpu.py to compare with the numpy
// restatement (under -fsanitize=address,undefined).  usage: selfcontact_host in.bin out.bin
//   in:  int32 T, 0; float64 tolerance, radii[24]; int32 parents[24]; uint64 mask[4]; float32 joints[T][24][3]
//   out: float64: the codes 24 i + j of tci_pair_of(0 .. 252); gap[T], closest[T]; rate, episodes, gap_min, the frame and the two
//        bones of self_closest, depth_mean; pair_frames[253]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "selfcontact_math.h"

static void need(bool ok, const char* what) {
    if (!ok) {
        fprintf(stderr, "selfcontact_host: %s\n", what);
        exit(2);
    }
}

int main(int argc, char** argv) {
    need(argc == 3, "usage: selfcontact_host in.bin out.bin");
    FILE* f = fopen(argv[1], "rb");
    need(f != NULL, "cannot open the input");
    int head[2], parents[TCG_J];
    double tolerance, radii[TCG_J];
    uint64_t mask[TCI_WORDS];
    need(fread(head, sizeof(int), 2, f) == 2 && fread(&tolerance, sizeof(double), 1, f) == 1 && fread(radii, sizeof(double), TCG_J, f) == TCG_J &&
             fread(parents, sizeof(int), TCG_J, f) == TCG_J && fread(mask, sizeof(uint64_t), TCI_WORDS, f) == TCI_WORDS,
         "short header");
    const int T = head[0];
    need(T >= 1 && T <= 100000 && tolerance >= 0.0, "bad sizes");
    for (int j = 1; j < TCG_J; ++j) need(parents[j] >= 0 && parents[j] < j, "bad parents");
    need((mask[3] >> (TCI_PAIRS - 192)) == 0 && (mask[0] | mask[1] | mask[2] | mask[3]) != 0, "bad mask");
    std::vector<float> J((size_t)T * TCG_J * 3);
    need(fread(J.data(), sizeof(float), J.size(), f) == J.size(), "short joints");
    fclose(f);

    std::vector<double> out;
    for (int k = 0; k < TCI_PAIRS; ++k) {
        int i, j;
        tci_pair_of(k, &i, &j);
        need(i >= 1 && i < j && j < TCG_J, "tci_pair_of left the range");
        out.push_back((double)(TCG_J * i + j));
    }
    std::vector<double> gap(T), code(T);
    std::vector<long> pair_frames(TCI_PAIRS, 0);
    for (int t = 0; t < T; ++t) {
        const float* P = J.data() + (size_t)t * TCG_J * 3;
        TcgBest best;
        best.v = 0.0;
        best.code = -1;
        for (int k = 0; k < TCI_PAIRS; ++k) {
            if (!tci_listed(mask, k)) continue;
            int i, j;
            tci_pair_of(k, &i, &j);
            const int pi = parents[i], pj = parents[j];
            const double d = tcg_seg_dist(tcg_v(P[3 * pi], P[3 * pi + 1], P[3 * pi + 2]), tcg_v(P[3 * i], P[3 * i + 1], P[3 * i + 2]),
                                          tcg_v(P[3 * pj], P[3 * pj + 1], P[3 * pj + 2]), tcg_v(P[3 * j], P[3 * j + 1], P[3 * j + 2]));
            TcgBest cand;
            cand.v = tcg_gap(d, radii[i], radii[j]);
            cand.code = TCG_J * i + j;
            pair_frames[k] += tci_contact(cand.v, tolerance);
            if (tci_before(cand, best)) best = cand;
        }
        gap[t] = best.v;
        code[t] = (double)best.code;
    }
    out.insert(out.end(), gap.begin(), gap.end());
    out.insert(out.end(), code.begin(), code.end());

    long n_con = 0, n_start = 0;
    TcgBest best;
    best.v = 0.0;
    best.code = -1;
    double lane[64];
    for (int l = 0; l < 64; ++l) lane[l] = 0.0;
    for (int t = 0; t < T; ++t) {
        const int con = tci_contact(gap[t], tolerance);
        n_con += con;
        n_start += con && !(t > 0 && tci_contact(gap[t - 1], tolerance));
        if (con) lane[t % 64] = tci_depth_add(lane[t % 64], gap[t]);
        if (tcg_finite(gap[t])) {
            TcgBest cand;
            cand.v = gap[t];
            cand.code = t;
            if (tcg_before_finite(cand, best)) best = cand;
        }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        double next[64];
        for (int l = 0; l < 64; ++l) next[l] = lane[l] + lane[l ^ o];
        for (int l = 0; l < 64; ++l) lane[l] = next[l];
    }
    const int bt = best.code, bc = bt < 0 ? 0 : (int)code[bt];
    out.push_back((double)n_con / (double)T);
    out.push_back((double)n_start);
    out.push_back(bt < 0 ? NAN : best.v);
    out.push_back((double)bt);
    out.push_back(bt < 0 ? -1.0 : (double)(bc / TCG_J));
    out.push_back(bt < 0 ? -1.0 : (double)(bc % TCG_J));
    out.push_back(n_con > 0 ? lane[0] / (double)n_con : NAN);
    for (int k = 0; k < TCI_PAIRS; ++k) out.push_back((double)pair_frames[k]);

    f = fopen(argv[2], "wb");
    need(f != NULL, "cannot open the output");
    need(fwrite(out.data(), sizeof(double), out.size(), f) == out.size(), "short write");
    fclose(f);
    return 0;
}
