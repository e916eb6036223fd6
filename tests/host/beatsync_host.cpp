// csrc/beatsync_math.h built for the host as a stand-alone program: the same functions the HIP kernels of csrc/beatsync.hip compile, run
// on whole clips the way the kernels run them (the lists in ascending order, a pick per music beat, the neighbour scan for the claims,
// the serial anchor pass, a slope per anchor, a frame at a time), printed for tests/test_beatsync_cpu.py to compare with the numpy
// restatement.  Built by the test with -fsanitize=address,undefined -ffp-contract=off.
//
//   beatsync_host in.bin
//
// in.bin: int32 b, dn, T, share, max_shift, has_contacts, rad; float64 max_rate, strength; float64 weights [2 rad + 1]; uint8 beats
// [b][T]; float32 joints [b][dn][T][24][3] (the input's joints, which the speed is taken from); float32 q [b][T dn][24][3], pos
// [b][T dn][3]; float32 contacts [b][dn][T][4] if has_contacts.
// stdout, one number per line (%.9g for a float32, %.17g for a float64, so that each is read back exactly): per warp status, kin_count,
// music_count, matched, dropped, anchors, rate_min_frame, rate_max_frame, shift_max, rate_min, rate_max, then warp [T], speed [T - 1],
// kin [T]; then per (clip, dancer) moved, copied; then q_out, pos_out and contacts_out in the layouts of their inputs.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "beatsync_math.h"

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
    std::vector<double> lim, weights;
    std::vector<uint8_t> beats;
    std::vector<float> joints, q, pos, contacts;
    if (!read_n(f, head, 7) || !read_n(f, lim, 2)) return 4;
    const int b = head[0], dn = head[1], T = head[2], share = head[3], max_shift = head[4], has_contacts = head[5], rad = head[6];
    if (b < 1 || dn < 1 || T < 1 || rad < 0) return 5;
    const size_t dancers = (size_t)b * dn;
    if (!read_n(f, weights, 2 * (size_t)rad + 1) || !read_n(f, beats, (size_t)b * T) || !read_n(f, joints, dancers * T * 72) ||
        !read_n(f, q, dancers * T * 72) || !read_n(f, pos, dancers * T * 3) || !read_n(f, contacts, has_contacts ? dancers * T * 4 : 0))
        return 6;
    fclose(f);
    const double max_rate = lim[0], strength = lim[1], nan = std::numeric_limits<double>::quiet_NaN();
    const int N = T - 1, W = share ? 1 : dn;
    std::vector<float> q_out(q.size()), pos_out(pos.size()), c_out(contacts.size());
    std::vector<int> moved(dancers), copied(dancers);
    for (int c = 0; c < b; ++c)
        for (int w = 0; w < W; ++w) {
            const int d_first = share ? 0 : w, d_count = share ? dn : 1;
            // the warp's curve: sized N, so that a read past it is a sanitizer error
            std::vector<double> pv(N), s(N);
            int status = 0;
            for (int t = 0; t < N; ++t) {
                double p = 0.0;
                for (int d = d_first; d < d_first + d_count; ++d) {
                    const float* J = joints.data() + (((size_t)c * dn + d) * T + t) * 72;
                    const double v = tcb_speed(J, J + 72);
                    p = share ? p + v : v;
                }
                if (share) p = p / (double)dn;
                pv[t] = p;
                status |= !tcb_finite(p);
            }
            for (int t = 0; t < N; ++t) s[t] = tcb_filter(pv.data(), N, weights.data(), rad, t);
            std::vector<int> kin(T, 0), kinL, musL;
            for (int t = 0; t < T; ++t)
                if (!status && tcb_is_min(s.data(), N, t)) {
                    kin[t] = 1;
                    kinL.push_back(t);
                }
            for (int t = 1; t <= T - 2; ++t)
                if (beats[(size_t)c * T + t]) musL.push_back(t);
            const int nk = (int)kinL.size(), nm = (int)musL.size();
            std::vector<int> pick(nm), cm, ck;
            for (int i = 0; i < nm; ++i) {
                int p = tcb_nearest(kinL.data(), nk, musL[i]);
                if (p >= 0 && (kinL[p] < musL[i] ? musL[i] - kinL[p] : kinL[p] - musL[i]) > max_shift) p = -1;
                pick[i] = p;
            }
            for (int i = 0; i < nm; ++i)
                if (tcb_keeps(musL.data(), pick.data(), kinL.data(), nm, i)) {
                    cm.push_back(musL[i]);
                    ck.push_back(kinL[pick[i]]);
                }
            const int nc = (int)cm.size();
            std::vector<int> am(nc + 2);
            std::vector<double> au(nc + 2), ae(nc + 2), ad(nc + 2, 0.0), warp(T);
            int dropped = 0;
            const int count = tcb_anchor_pass(cm.data(), ck.data(), nc, T, strength, max_rate, am.data(), au.data(), ae.data(), &dropped);
            if (count > 2)
                for (int k = 0; k < count; ++k) ad[k] = tcc_slope(am.data(), au.data(), count, k) - 1.0;
            for (int t = 0; t < T; ++t) warp[t] = tcb_warp(am.data(), ae.data(), ad.data(), count, T, t);
            double shift = 0.0;
            int n_moved = 0;
            TccPeak lo, hi;
            lo.v = hi.v = 0.0;
            lo.t = hi.t = -1;
            for (int t = 0; t < T; ++t) {
                shift = fmax(shift, fabs(warp[t] - (double)t));
                n_moved += warp[t] != (double)t;
                if (t < N) {
                    TccPeak r;
                    r.v = warp[t + 1] - warp[t];
                    r.t = t;
                    if (tcc_smaller(r, lo)) lo = r;
                    if (tcc_larger(r, hi)) hi = r;
                }
            }
            printf("%d\n%d\n%d\n%d\n%d\n%d\n%d\n%d\n%.17g\n%.17g\n%.17g\n", status, nk, nm, nc, dropped, count - 2, lo.t, hi.t, shift,
                   lo.t < 0 ? nan : lo.v, hi.t < 0 ? nan : hi.v);
            for (int t = 0; t < T; ++t) printf("%.17g\n", warp[t]);
            for (int t = 0; t < N; ++t) printf("%.17g\n", status ? nan : s[t]);
            for (int t = 0; t < T; ++t) printf("%d\n", kin[t]);
            // the resampling of the warp's dancers
            for (int d = d_first; d < d_first + d_count; ++d) {
                const size_t seq = (size_t)c * dn + d;
                int n_copied = 0;
                for (int t = 0; t < T; ++t) {
                    double a;
                    const int i = tcb_source(warp[t], T, &a);
                    const size_t row = ((size_t)c * T + t) * dn + d, r0 = ((size_t)c * T + i) * dn + d, r1 = a != 0.0 ? r0 + dn : r0;
                    for (int j = 0; j < TCB_J; ++j) {
                        const float *self = q.data() + row * 72 + 3 * j, *x = q.data() + r0 * 72 + 3 * j, *y = q.data() + r1 * 72 + 3 * j;
                        float* dst = q_out.data() + row * 72 + 3 * j;
                        if (a == 0.0) {
                            dst[0] = x[0]; dst[1] = x[1]; dst[2] = x[2];
                        } else if (tcb_finite3(x) && tcb_finite3(y)) {
                            const TckV r = tcb_slerp(x, y, a);
                            dst[0] = (float)r.x; dst[1] = (float)r.y; dst[2] = (float)r.z;
                        } else {
                            dst[0] = self[0]; dst[1] = self[1]; dst[2] = self[2];
                            ++n_copied;
                        }
                    }
                    const float *self = pos.data() + row * 3, *x = pos.data() + r0 * 3, *y = pos.data() + r1 * 3;
                    float* dst = pos_out.data() + row * 3;
                    if (a == 0.0) {
                        dst[0] = x[0]; dst[1] = x[1]; dst[2] = x[2];
                    } else if (tcb_finite3(x) && tcb_finite3(y)) {
                        for (int k = 0; k < 3; ++k) dst[k] = (float)tcb_lerp(x[k], y[k], a);
                    } else {
                        dst[0] = self[0]; dst[1] = self[1]; dst[2] = self[2];
                        ++n_copied;
                    }
                    if (has_contacts)
                        for (int k = 0; k < 4; ++k) c_out[(seq * T + t) * 4 + k] = contacts[(seq * T + (a < 0.5 ? i : i + 1)) * 4 + k];
                }
                moved[seq] = n_moved;
                copied[seq] = n_copied;
            }
        }
    for (size_t seq = 0; seq < dancers; ++seq) printf("%d\n%d\n", moved[seq], copied[seq]);
    for (float v : q_out) printf("%.9g\n", v);
    for (float v : pos_out) printf("%.9g\n", v);
    for (float v : c_out) printf("%.9g\n", v);
    return 0;
}
