// csrc/smooth_math.h (with csrc/footlock_math.h) built for the host as a stand-alone program: the same functions the HIP kernels of
// csrc/smooth.hip compile, run on one dancer's frames the way the kernels run them, printed for tests/test_smooth_cpu.py to compare
// with the numpy restatement.  Built by the test with -fsanitize=address,undefined -ffp-contract=off.
//
//   smooth_host in.bin
//
// in.bin: int32 T, W, Wr, mask; float64 taps [W][W], root_taps [Wr][Wr]; float32 q [T][24][3], pos [T][3].
// stdout, one number per line (%.17g, so that every float64 is read back exactly): per frame the three filtered root components and
// the copied flag; per frame and joint the three components of the filtered rotation vector and the copied flag (a copied output
// prints the input); per frame and joint the change between the input and the float32 rounding of the output; then the acceleration
// terms of the root track (T - 2) and its jerk terms (T - 3) at 30 fps; then the frame of the largest acceleration by tcw_beats.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "smooth_math.h"

template <class X>
static bool read_n(FILE* f, std::vector<X>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(X), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<int32_t> head;
    std::vector<double> taps, root_taps;
    std::vector<float> q, pos;
    if (!read_n(f, head, 4)) return 4;
    const int T = head[0], W = head[1], Wr = head[2];
    const unsigned mask = (unsigned)head[3];
    if (T < 4 || W < 3 || Wr < 3 || W > T || Wr > T || !(W & 1) || !(Wr & 1)) return 5;
    if (!read_n(f, taps, (size_t)W * W) || !read_n(f, root_taps, (size_t)Wr * Wr) || !read_n(f, q, (size_t)T * TCW_J * 3) ||
        !read_n(f, pos, (size_t)T * 3))
        return 6;
    fclose(f);

    // the rows the filter kernel stages: one per joint and component over the frames, and the root's three
    std::vector<double> Q((size_t)TCW_J * 4 * T), P((size_t)3 * T);
    for (int t = 0; t < T; ++t) {
        for (int j = 0; j < TCW_J; ++j) {
            const TckQ v = tck_quat(&q[((size_t)t * TCW_J + j) * 3]);
            double* dst = &Q[(size_t)j * 4 * T + t];
            dst[0] = v.w; dst[T] = v.x; dst[2 * (size_t)T] = v.y; dst[3 * (size_t)T] = v.z;
        }
        for (int k = 0; k < 3; ++k) P[(size_t)k * T + t] = (double)pos[(size_t)t * 3 + k];
    }
    for (int t = 0; t < T; ++t) {
        const int s = tcw_start(t, T, Wr);
        const double* tap = &root_taps[(size_t)(t - s) * Wr];
        double v[3];
        bool ok = true;
        for (int k = 0; k < 3; ++k) {
            v[k] = tcw_tap_sum(tap, &P[(size_t)k * T + s], Wr);
            ok = ok && tcw_finite(v[k]);
        }
        for (int k = 0; k < 3; ++k) printf("%.17g\n", ok ? v[k] : (double)pos[(size_t)t * 3 + k]);
        printf("%d\n", ok ? 0 : 1);
    }
    std::vector<float> out((size_t)T * TCW_J * 3);
    for (int t = 0; t < T; ++t) {
        const int s = tcw_start(t, T, W);
        const double* tap = &taps[(size_t)(t - s) * W];
        for (int j = 0; j < TCW_J; ++j) {
            const float* src = &q[((size_t)t * TCW_J + j) * 3];
            float* dst = &out[((size_t)t * TCW_J + j) * 3];
            TcwRot r;
            r.copied = 1;
            r.r = tck_v(0.0, 0.0, 0.0);
            const bool listed = (mask >> j) & 1u;
            if (listed) r = tcw_filter_quat(tap, &Q[(size_t)j * 4 * T + s], T, W, t - s);
            if (r.copied) {
                for (int k = 0; k < 3; ++k) dst[k] = src[k];
                printf("%.17g\n%.17g\n%.17g\n%d\n", (double)src[0], (double)src[1], (double)src[2], listed ? 1 : 0);
            } else {
                dst[0] = (float)r.r.x; dst[1] = (float)r.r.y; dst[2] = (float)r.r.z;
                printf("%.17g\n%.17g\n%.17g\n0\n", r.r.x, r.r.y, r.r.z);
            }
        }
    }
    for (size_t e = 0; e < (size_t)T * TCW_J; ++e) printf("%.17g\n", tcw_rot_change(&q[e * 3], &out[e * 3]));
    TcwPeak top;
    top.v = 0.0;
    top.t = top.j = -1;
    for (int t = 1; t < T - 1; ++t) {
        TcwPeak cand;
        cand.t = t;
        cand.j = 0;
        cand.v = tcw_accel(tcw_point(&pos[(size_t)(t - 1) * 3]), tcw_point(&pos[(size_t)t * 3]), tcw_point(&pos[(size_t)(t + 1) * 3]), 900.0);
        printf("%.17g\n", cand.v);
        if (tcw_finite(cand.v) && tcw_beats(cand, top)) top = cand;
    }
    for (int t = 1; t < T - 2; ++t)
        printf("%.17g\n", tcw_jerk(tcw_point(&pos[(size_t)(t - 1) * 3]), tcw_point(&pos[(size_t)t * 3]), tcw_point(&pos[(size_t)(t + 1) * 3]),
                                   tcw_point(&pos[(size_t)(t + 2) * 3]), 27000.0));
    printf("%d\n", top.t);
    return 0;
}
