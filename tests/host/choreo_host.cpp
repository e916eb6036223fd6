// csrc/choreo_math.h built for the host as a stand-alone program: the same functions the HIP kernels of csrc/choreo.hip compile, run
// on a whole plan the way the kernels run them (the steps of a dancer summed per lane, the extrema by the total orders), printed for
// tests/test_choreo_cpu.py to compare with the numpy restatement.  Built by the test with -fsanitize=address,undefined
// -ffp-contract=off.
//
//   choreo_host in.bin
//
// in.bin: int32 b, dn, K, frames, keys_per_dancer, has_counts, has_norm; float64 fps, min_distance, max_speed; float32 scale [2],
// min_ [2]; int32 keys [K] or [b][dn][K]; int32 counts [b][dn] if has_counts; float32 points [b][dn][K][2].
// stdout, one number per line (%.9g for a float32, %.17g for a float64, so that each is read back exactly): per (clip, dancer) status,
// clamped, speed_max, speed_peak, too_fast, path_length; then traj [b][dn][frames][2]; then x0 [b][frames dn][3]; then per (clip,
// pair) dist_min, dist_min_frame, too_close.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "choreo_math.h"

template <class X>
static bool read_n(FILE* f, std::vector<X>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(X), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<int32_t> head, keys, counts;
    std::vector<double> lim;
    std::vector<float> norm, points;
    if (!read_n(f, head, 7) || !read_n(f, lim, 3) || !read_n(f, norm, 4)) return 4;
    const int b = head[0], dn = head[1], K = head[2], frames = head[3], per_dancer = head[4], has_counts = head[5], has_norm = head[6];
    if (b < 1 || dn < 1 || K < 1 || K > 256 || frames < 1) return 5;
    const size_t dancers = (size_t)b * dn;
    if (!read_n(f, keys, per_dancer ? dancers * K : (size_t)K) || !read_n(f, counts, has_counts ? dancers : 0) ||
        !read_n(f, points, dancers * K * 2))
        return 6;
    fclose(f);
    const double fps = lim[0], min_distance = lim[1], max_speed = lim[2];
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const float nanf = std::numeric_limits<float>::quiet_NaN();
    std::vector<float> traj(dancers * frames * 2), x0(dancers * frames * 3, 0.0f);
    for (size_t seq = 0; seq < dancers; ++seq) {
        const size_t c = seq / dn, d = seq % dn;
        const int count = has_counts ? counts[seq] : K;
        const int32_t* key = keys.data() + (per_dancer ? seq * K : 0);
        const float* pt = points.data() + seq * K * 2;
        float* tr = traj.data() + seq * frames * 2;
        float* xo = x0.data() + (c * frames * dn + d) * 3;
        int bad_key = count < 1 || count > K, bad_point = 0;
        std::vector<int> skey;
        std::vector<double> y[2], sl[2];
        for (int k = 0; !bad_key && k < count; ++k) {         // sized by count: a read of the padding is a sanitizer error
            skey.push_back(key[k]);
            y[0].push_back((double)pt[2 * k]);
            y[1].push_back((double)pt[2 * k + 1]);
        }
        for (int k = 0; k < (int)skey.size(); ++k) {
            bad_key = bad_key || skey[k] < 0 || skey[k] >= frames || (k > 0 && skey[k - 1] >= skey[k]);
            bad_point = bad_point || !(tcc_finite(y[0][k]) && tcc_finite(y[1][k]));
        }
        if (bad_key || bad_point) {
            for (int t = 0; t < frames; ++t) {
                tr[2 * t] = tr[2 * t + 1] = nanf;
                xo[(size_t)t * dn * 3] = xo[(size_t)t * dn * 3 + 1] = nanf;
            }
            printf("%d\n0\nnan\n-1\n0\nnan\n", bad_key ? 1 : 2);
            continue;
        }
        for (int c2 = 0; c2 < 2; ++c2)
            for (int k = 0; k < count; ++k) sl[c2].push_back(tcc_slope(skey.data(), y[c2].data(), count, k));
        int n_clamped = 0, n_fast = 0;
        for (int t = 0; t < frames; ++t) {
            const double vx = tcc_eval(skey.data(), y[0].data(), sl[0].data(), count, t), vy = tcc_eval(skey.data(), y[1].data(), sl[1].data(), count, t);
            tr[2 * t] = (float)vx;
            tr[2 * t + 1] = (float)vy;
            float* o = xo + (size_t)t * dn * 3;
            int hit = 0;
            o[0] = has_norm ? (float)tcc_x0(vx, (double)norm[0], (double)norm[2], &hit) : tr[2 * t];
            o[1] = has_norm ? (float)tcc_x0(vy, (double)norm[1], (double)norm[3], &hit) : tr[2 * t + 1];
            n_clamped += hit;
        }
        double lanes[64];
        for (int l = 0; l < 64; ++l) lanes[l] = 0.0;
        TccPeak top;
        top.v = 0.0; top.t = -1;
        for (int t = 0; t < frames - 1; ++t) {
            const double step = tcc_dist(tr[2 * t], tr[2 * t + 1], tr[2 * t + 2], tr[2 * t + 3]);
            if (!tcc_finite(step)) continue;
            lanes[t % 64] = lanes[t % 64] + step;
            TccPeak cand;
            cand.v = step * fps; cand.t = t;
            if (tcc_larger(cand, top)) top = cand;
            n_fast += cand.v > max_speed;
        }
        double total = 0.0;
        for (int l = 0; l < 64; ++l) total = total + lanes[l];
        printf("0\n%d\n%.17g\n%d\n%d\n%.17g\n", n_clamped, top.t < 0 ? nan : top.v, top.t, n_fast, total);
    }
    for (float v : traj) printf("%.9g\n", (double)v);
    for (float v : x0) printf("%.9g\n", (double)v);
    const int pairs = dn * (dn - 1) / 2;
    for (int c = 0; c < b; ++c)
        for (int p = 0; p < pairs; ++p) {
            int i, j;
            tcc_pair(p, dn, &i, &j);
            const float* A = traj.data() + ((size_t)c * dn + i) * frames * 2;
            const float* B = traj.data() + ((size_t)c * dn + j) * frames * 2;
            TccPeak low;
            low.v = 0.0; low.t = -1;
            int n_close = 0;
            for (int t = 0; t < frames; ++t) {
                TccPeak cand;
                cand.v = tcc_dist(A[2 * t], A[2 * t + 1], B[2 * t], B[2 * t + 1]);
                cand.t = t;
                if (!tcc_finite(cand.v)) continue;
                if (tcc_smaller(cand, low)) low = cand;
                n_close += cand.v < min_distance;
            }
            printf("%.17g\n%d\n%d\n", low.t < 0 ? nan : low.v, low.t, n_close);
        }
    return 0;
}
