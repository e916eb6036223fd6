// Host build (g++ -ffp-contract=off) of tcdiff_amd/csrc/geo_math.h: the per-frame points and predicates the HIP kernel of
// csrc/geometric.hip calls, exported for tests/test_geometric_cpu.py (compared there with the numpy restatement).
#include "geo_math.h"

extern "C" {
// one dancer's joints [T][24][3] -> counts[R]: the number of frames t = 1 .. T - 1 at which each row holds
void host_geometric_counts(const float* joints, int T, int up, const int* table, const double* range, int R, double tau,
                           long* counts) {
    for (int r = 0; r < R; ++r) {
        GeoRow row;
        row.kind = table[5 * r];
        row.a = table[5 * r + 1];
        row.b = table[5 * r + 2];
        row.c = table[5 * r + 3];
        row.p = table[5 * r + 4];
        row.lo = range[2 * r];
        row.hi = range[2 * r + 1];
        counts[r] = 0;
        if (!geo_row_valid(row.kind, row.a, row.b, row.c, row.p)) continue;
        for (int t = 1; t < T; ++t) {
            const float* F = joints + 72L * t;
            counts[r] += geo_holds(row, F, geo_floor(F, up), F - 72, geo_floor(F - 72, up), up, tau);
        }
    }
}
}
