/* tcdiff_apart.h -- the ninth header of libtcdiff_gfx950.so's C ABI: KEEPING THE DANCERS' BODIES APART.  A post-process on what
 * tcdiff_pose_export (or tck_foot_lock) leaves on the device: each dancer's root is shifted HORIZONTALLY, as little as the capsule
 * bodies of tcdiff_group.h require, the shift eased in and out in time; rotations are untouched, and the launch reports what it did
 * and what it could not do.  The conventions of tcdiff_hip.h hold: every function returns 0 or a negative TC_ERR_* code, nothing is
 * allocated, nothing synchronises the host, pointers are caller-owned DEVICE pointers (`joint_strides`, `parents`, `radii`,
 * `mobility` and `bytes` excepted: HOST), work is enqueued on `stream`, the checks precede any GPU call.
 *
 * Why the functions are tcp_*: the sets of tcdiff_*, tcx_*, tcs_*, tcr_*, tcj_*, tck_* and tcg_* symbols the library exports are
 * frozen (the tests hold each equal to the built library's dynamic symbols).  This header takes a prefix of its own;
 * tcdiff_amd/_lib.py binds it as APART next to ABI, EXT, GLTF, SKIN, SHADE, MJPEG, FOOTLOCK and GROUP and adds it to none of them
 * nor to EXPORTS.
 *
 * The reference has no counterpart (it renders the raw poses); the construction is the project's own, parity with any other tool
 * is unpinned, and what follows is the definition.  csrc/apart_math.h is its arithmetic, tests/apart_ref.py its numpy restatement.
 * margin, iterations, rounds, blend and max_push are choices, not measurements.
 * What the construction does not promise: with three or more dancers a push that clears one pair can close another; further rounds
 * reduce that but need not end it, and contact_after says what is left.  Dancers that walk through each other are not repaired by
 * a shift of at most max_push; `capped` counts those frames.
 * Not built: vertical moves; changing a pose to dodge; resolving inside the sampler; mesh-level contact; contact between parts of
 * one dancer; smoothing beyond the envelope.
 *
 * ---- input ----------------------------------------------------------------------------------------------------------------------
 * joints: float32, read in place as in tcdiff_group.h: joint j, component k of (clip c, dancer d, frame t) is at
 * joints + c strides[0] + d strides[1] + t strides[2] + 3 j + k (element strides, each >= 0).  pos: float32 [b][T dn][3], row =
 * frame dn + dancer, contiguous.  The pairs (a, b), a < b, their order, P, dist, gap, the bones, `parents` and `radii` and the total
 * order of a minimum (a NaN first) are exactly those of tcdiff_group.h; gap(Ja, Jb) below is its per-frame body gap of two sets of 24
 * joints given as float64.  All arithmetic is float64 on the float32 inputs, every product and sum rounded on its own (no
 * contraction).  The floor components f0 < f1 are the two components that are not `up`.
 *
 * ---- the definition -------------------------------------------------------------------------------------------------------------
 * State: the shift plane S[c, d, t] = (S0, S1), two float64, the shift of the floor components f0 and f1; it starts at 0.
 * mobility[d] >= 0 says how a pair's push is shared: wa = mobility[a] / (mobility[a] + mobility[b]), wb = 1 - wa; if both are 0 the
 * pair is "pinned": its m below is 0 in every frame (its entry gap is still evaluated).
 * `rounds` rounds follow, each of two steps.
 *
 * Step 1, demand, per (clip, pair (a, b), frame t):
 *   Ja[j] = float64(J_a[j]) with S[a, t] added to its floor components (the `up` component as it is), Jb likewise.
 *   d = (Jb[0].f0 - Ja[0].f0, Jb[0].f1 - Ja[0].f1), n2 = d0 d0 + d1 d1.  If n2 > 1e-18 (false for a NaN): n = sqrt(n2),
 *   u = (d0 / n, d1 / n); else u = (1, 0).
 *   g(m) = gap(Ja', Jb') where, with qa = wa m and qb = wb m, the floor components of every joint are Ja'.f = Ja.f - qa u_f and
 *   Jb'.f = Jb.f + qb u_f: each formed from the unmoved Ja, Jb on every evaluation, never accumulated.
 *   m = 0, g = g(0), the frame's ENTRY GAP.  Unless the pair is pinned, repeat at most `iterations` times:
 *     need = margin - g;  stop unless need > 0 (a NaN gap stops: m stays 0);
 *     m = min(m + need, max_push);  g = g(m);  if m == max_push: the frame is CAPPED in this round, stop.
 *   The frame is PUSHED in this round if m > 0.  The entry gap of round 1 is the "before" gap.
 * Step 2, combine:
 *   e_p[t] = max over t', |t' - t| <= blend, 0 <= t' < T, of m_p[t'] (1 - |t - t'| / (blend + 1)), the quotient and the difference
 *   in float64 -- a maximum of exact candidates, so its order is free; never below m_p[t]; it fades linearly over `blend` frames.
 *   For every dancer the pairs that contain it, in ascending pair order:
 *     S[a, t] = S[a, t] - (wa e_p[t]) u_p[t]   and   S[b, t] = S[b, t] + (wb e_p[t]) u_p[t],   component by component.
 *
 * Output: where both components of the final S[c, d, t] are 0, the output words of that (clip, dancer, frame) -- its row of pos_out
 * and its 24 joints -- are the input's words, copied without arithmetic (a NaN keeps its payload).  Elsewhere each floor component x
 * of pos and of the 24 joints is float32(float64(x) + S); the `up` component is always the input's word.
 * "after": the entry gap of the demand step with S = 0, evaluated on the float32 joints_out.
 * Per (clip, pair), over its T frames:  contact_before / contact_after = the frames whose before / after gap is < 0;
 *   gap_min_before / gap_min_after = the smallest finite such gap, NaN if there is none;  pushed / capped = the frames that some
 *   round pushed / capped.  With rounds = 0 the output is the input and "before" is "after".
 * Per (clip, dancer):  max_shift = max over t of sqrt(S0 S0 + S1 S1);  max_step = max over t >= 1 of the same length of
 *   S[t] - S[t - 1], 0 for T = 1.
 *
 * ---- the launchers (csrc/apart.hip) -----------------------------------------------------------------------------------------------
 * TC_APART_LAUNCHES(rounds) launches whatever b is; no atomics, every sum in one order, every minimum over a total order: the same
 * input gives the same bits.
 *   demand  (per round): one wave per (clip, pair, frame), four frames per workgroup of 256; both dancers' shifted joints staged in
 *           LDS as float64; each evaluation of g puts the 529 bone pairs over the lanes in nine rounds, then a cross-lane minimum of
 *           (gap, code); the iteration's exit is wave-uniform, a frame without contact costs one evaluation.  Writes m and u, in
 *           round 1 the before gap, and ORs the two flags into one byte per (pair, frame): each byte has one owner, lane 0 of its wave.
 *   combine (per round): one thread per (clip, dancer, frame): the envelopes of its pairs from the m planes, S updated.
 *   apply:  one thread per (clip, dancer, frame, row), the 24 joints and the row of pos: the copy rule above.
 *   verify: the demand kernel with zero iterations on joints_out: the after gap.
 *   stats:  one workgroup per (clip, pair) and one per (clip, dancer): integer counts, the finite minimum, the maxima, over T.
 * workspace: TC_APART_WS_PAIR_FRAME bytes per (clip, pair, frame) -- m, u, the two gap planes (float64) and the flag byte -- and
 * TC_APART_WS_DANCER_FRAME per (clip, dancer, frame) -- S, used when `shift` is NULL --, rounded up to a multiple of 8; aligned to 8.
 *
 * The checks, in this order.  TC_ERR_ARG: a NULL pointer (shift may be NULL); b < 1, dn < 2 or T < 1; up outside 0..2; iterations,
 * rounds or blend negative; margin or max_push negative or not finite.  TC_ERR_UNSUPPORTED: dn > TC_APART_MAX_DANCERS; blend >
 * TC_APART_MAX_BLEND; rounds > TC_APART_MAX_ROUNDS; more than 2^31 - 1 (clip, pair, frame) triples or (clip, dancer, frame, row)
 * items, 25 rows each.  TC_ERR_ARG: a negative stride; a parent of joint 1 .. 23 that is negative or does not precede its child; a
 * radius of bone 1 .. 23 that is negative or not finite; a mobility that is negative or not finite; workspace_bytes below
 * tcp_keep_apart_workspace's.  TC_ERR_ALIGN: workspace or shift not aligned to 8 bytes.
 * tcp_keep_apart_workspace: TC_ERR_ARG for a NULL `bytes`, the same shape checks, TC_ERR_UNSUPPORTED likewise. */
#ifndef TCDIFF_APART_H
#define TCDIFF_APART_H

#include "tcdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TC_APART_LAUNCHES(rounds) (2 * (rounds) + 3)
#define TC_APART_MAX_DANCERS 32
#define TC_APART_MAX_BLEND 65536
#define TC_APART_MAX_ROUNDS 64
#define TC_APART_WS_PAIR_FRAME 41
#define TC_APART_WS_DANCER_FRAME 16
#define TC_APART_PUSHED 1
#define TC_APART_CAPPED 2

/* bytes[0] (a HOST long) = the workspace tcp_keep_apart needs for b clips of dn dancers and T frames */
int tcp_keep_apart_workspace(int b, int dn, int T, long* bytes);

/* pos_out [b][T dn][3] and joints_out [b][dn][T][24][3] float32; shift [b][dn][T][2] float64, the final S, or NULL.
 * contact_before, contact_after, pushed, capped [b P] int64 (long); gap_min_before, gap_min_after [b P] float64;
 * max_shift, max_step [b dn] float64. */
int tcp_keep_apart(const float* pos, const float* joints, const long* joint_strides, int b, int dn, int T, int up,
                   const int* parents, const double* radii, const double* mobility, double margin, int iterations, int rounds,
                   int blend, double max_push, void* workspace, long workspace_bytes, float* pos_out, float* joints_out,
                   double* shift, long* contact_before, long* contact_after, double* gap_min_before, double* gap_min_after,
                   long* pushed, long* capped, double* max_shift, double* max_step, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TCDIFF_APART_H */
