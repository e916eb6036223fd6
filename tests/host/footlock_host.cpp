// csrc/footlock_math.h built for the host as a stand-alone program (tests/test_footlock_cpu.py; g++ -ffp-contract=off):
//   footlock_host <in> <out>
// <in>:  int32 b, dn, T, has_contacts, blend; float32 contact_threshold; float64 still, reach; float32 offsets[24][3],
//        q[b][T dn][24][3], pos[b][T dn][3], and contacts[b][dn][T][4] if has_contacts
// <out>: float64 q64[b][T dn][2][3][3] (per leg hip, knee, ankle: the solved rotation vectors before their rounding, or the input's),
//        float64 d[b][dn][2][T][3], max_shift[b][dn][2], int32 status[b][dn][2][T], planted[b][dn][2], clamped[b][dn][2]
// The per-frame functions are the kernels'; the runs are walked frame by frame here, with none of the kernels' chunks.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "footlock_math.h"

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
template <class V> static bool write_all(FILE* f, const V& v) { return v.empty() || fwrite(v.data(), sizeof(v[0]), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 3;
    int32_t head[5];
    float thr, offsets[72];
    double par[2];
    if (!read_all(in, head, sizeof head) || !read_all(in, &thr, sizeof thr) || !read_all(in, par, sizeof par) || !read_all(in, offsets, sizeof offsets))
        return 4;
    const int b = head[0], dn = head[1], T = head[2], has = head[3], blend = head[4];
    if (b < 1 || dn < 1 || T < 1 || blend < 0) return 4;
    const double still = par[0], reach = par[1];
    const size_t rows = (size_t)b * T * dn, seqs = (size_t)b * dn * 2;
    std::vector<float> q(rows * 72), pos(rows * 3), contacts(has ? rows * 4 : 0);
    if (!read_all(in, q.data(), 4 * q.size()) || !read_all(in, pos.data(), 4 * pos.size()) || !read_all(in, contacts.data(), 4 * contacts.size())) return 4;
    fclose(in);

    std::vector<double> q64(rows * 18), dout(seqs * T * 3), max_shift(seqs, 0.0);
    std::vector<int32_t> status(seqs * T, 0), planted(seqs, 0), clamped(seqs, 0);
    std::vector<TckLeg> legs((size_t)T);
    std::vector<TckQ> R0((size_t)T);
    std::vector<TckV> d((size_t)T);
    std::vector<int> g((size_t)T);
    for (int c = 0; c < b; ++c)
        for (int dd = 0; dd < dn; ++dd)
            for (int leg = 0; leg < 2; ++leg) {
                float off[12];
                for (int k = 0; k < 4; ++k)
                    for (int x = 0; x < 3; ++x) off[3 * k + x] = offsets[3 * (1 + leg + 3 * k) + x];
                const double l1 = tck_bone(off + 3), l2 = tck_bone(off + 6);
                const size_t seq = ((size_t)c * dn + dd) * 2 + leg;
                for (int t = 0; t < T; ++t) {
                    const size_t row = ((size_t)c * T + t) * dn + dd;
                    const float* a = &q[row * 72];
                    R0[t] = tck_quat(a);
                    legs[t] = tck_leg_fk(R0[t], tck_v(pos[row * 3], pos[row * 3 + 1], pos[row * 3 + 2]), a + 3 * (1 + leg), a + 3 * (4 + leg),
                                         a + 3 * (7 + leg), off);
                }
                for (int t = 0; t < T; ++t) {
                    bool ca, ce;
                    if (has) {
                        const float* k = &contacts[(((size_t)c * dn + dd) * T + t) * 4];
                        ca = k[leg] > thr;
                        ce = k[2 + leg] > thr;
                    } else if (t == T - 1) {
                        ca = ce = true;
                    } else {
                        ca = tck_norm(tck_sub(legs[t + 1].Pa, legs[t].Pa)) < still;
                        ce = tck_norm(tck_sub(legs[t + 1].Pe, legs[t].Pe)) < still;
                    }
                    g[t] = ca ? 1 : (ce ? 2 : 0);
                    planted[seq] += g[t] != 0;
                }
                for (int t = 0; t < T;) {
                    if (!g[t]) {
                        ++t;
                        continue;
                    }
                    int end = t;
                    while (end + 1 < T && g[end + 1] == g[t]) ++end;
                    TckV s = tck_v(0.0, 0.0, 0.0);
                    for (int u = t; u <= end; ++u) s = tck_add(s, g[t] == 1 ? legs[u].Pa : legs[u].Pe);
                    const TckV A = tck_over(s, (double)(end - t + 1));
                    for (int u = t; u <= end; ++u) d[u] = tck_sub(A, g[t] == 1 ? legs[u].Pa : legs[u].Pe);
                    t = end + 1;
                }
                for (int t = 0; t < T; ++t) {
                    if (g[t]) continue;
                    int t0 = t - 1, t1 = t + 1;
                    while (t0 >= 0 && !g[t0]) --t0;
                    while (t1 < T && !g[t1]) ++t1;
                    if (t1 >= T) t1 = -1;
                    const TckV z = tck_v(0.0, 0.0, 0.0);
                    d[t] = tck_ease(t, t0, t1, t0 >= 0 ? d[t0] : z, t1 >= 0 ? d[t1] : z, blend);
                }
                for (int t = 0; t < T; ++t) {
                    const size_t row = ((size_t)c * T + t) * dn + dd;
                    double rp = 0.0;
                    clamped[seq] += tck_reach(legs[t].Ph, legs[t].Pa, d[t], l1, l2, reach, &rp) == 2;
                    const TckSolve s = tck_solve(R0[t], legs[t], d[t], l1, l2, reach);
                    status[seq * T + t] = s.status;
                    const TckV out[3] = {s.qh, s.qk, s.qa};
                    for (int k = 0; k < 3; ++k) {
                        const float* a = &q[row * 72 + 3 * (1 + leg + 3 * k)];
                        double* o = &q64[row * 18 + leg * 9 + 3 * k];
                        o[0] = s.status ? out[k].x : (double)a[0];
                        o[1] = s.status ? out[k].y : (double)a[1];
                        o[2] = s.status ? out[k].z : (double)a[2];
                    }
                    const double n = tck_norm(d[t]);
                    if (n > max_shift[seq]) max_shift[seq] = n;
                    dout[(seq * T + t) * 3] = d[t].x;
                    dout[(seq * T + t) * 3 + 1] = d[t].y;
                    dout[(seq * T + t) * 3 + 2] = d[t].z;
                }
            }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 5;
    const bool ok = write_all(out, q64) && write_all(out, dout) && write_all(out, max_shift) && write_all(out, status) && write_all(out, planted) &&
                    write_all(out, clamped);
    return fclose(out) == 0 && ok ? 0 : 6;
}
