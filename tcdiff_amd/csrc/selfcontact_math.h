// What the self-contact metric (include/tcdiff_selfcontact.h) adds to the arithmetic of the group metrics (csrc/group_math.h, which
// holds the distance of two segments, the gap of two capsules and the orders of the minima): the numbering of the 253 bone pairs of
// one dancer, the test of a pair's bit in the mask, the minimum over candidates some of which are absent, and the tests against the
// tolerance, as plain functions (no memory traffic of their own, no HIP builtins), so that the same source compiles
//   * as __device__ code into libtcdiff_gfx950.so (csrc/selfcontact.hip), and
//   * as host code under g++ (tests/host/selfcontact_host.cpp), checked on the CPU against the numpy restatement
//     (tests/test_selfcontact_cpu.py) before it ever runs on a GPU.
#pragma once
#include <stdint.h>

#include "group_math.h"

#define TCI_PAIRS 253                     // 23 * 22 / 2 unordered pairs (i, j), 1 <= i < j <= 23
#define TCI_WORDS 4                       // 64-bit words of a mask or of a frame's penetration bits

// pair k = 0 .. 252 in lexicographic order -> (i, j), in closed form.  Counted from the end, r = 252 - k, the rows have 1, 2, ... 22
// entries: row m = 22 - i starts at m (m + 1) / 2, so m = floor((sqrt(8 r + 1) - 1) / 2).  The floor steps where 8 r + 1 is an odd
// square; 8 r + 5 lies at least 4 from every odd square on either side (the values 8 r + 1 are 8 apart), which is 4 / (2 * 45) of
// the root at the least: no rounding of a float square root comes near it.
TC_HD void tci_pair_of(int k, int* i, int* j) {
    const int r = TCI_PAIRS - 1 - k;
    const int m = (int)((sqrtf((float)(8 * r + 5)) - 1.0f) * 0.5f);
    *i = 22 - m;
    *j = 23 - (r - m * (m + 1) / 2);
}

TC_HD int tci_listed(const uint64_t* mask, int k) { return (int)((mask[k >> 6] >> (k & 63)) & 1u); }

// tcg_before among candidates of which some are absent (code < 0: the lane's pair is not listed): a present one precedes an absent one
TC_HD int tci_before(TcgBest a, TcgBest b) {
    if (a.code < 0 || b.code < 0) return b.code < 0 && a.code >= 0;
    return tcg_before(a, b);
}

// strictly deeper than the tolerance; false for a NaN
TC_HD int tci_contact(double gap, double tolerance) { return gap < -tolerance; }

// one term of the depth sum
TC_HD double tci_depth_add(double sum, double gap) { TCG_NO_CONTRACT return sum + (-gap); }
