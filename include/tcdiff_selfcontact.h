/* tcdiff_selfcontact.h -- the twelfth header of libtcdiff_gfx950.so's C ABI: does a dancer pass through ITSELF?  A forearm through the
 * chest, a hand through the head, a shin through the other thigh: the contact of two capsules of ONE dancer, measured per clip and
 * dancer from the joint positions that tcdiff_pose_export (or tck_foot_lock, tcp_keep_apart, tcf_ground) leaves on the device.  The
 * conventions of tcdiff_hip.h and tcdiff_group.h hold: every function returns 0 or a negative TC_ERR_* code, nothing is allocated,
 * nothing synchronises the host, pointers are caller-owned DEVICE pointers (`joint_strides`, `parents`, `radii`, `mask` and `bytes`
 * excepted: HOST), work is enqueued on `stream`, the checks precede any GPU call.
 *
 * Why the functions are tci_*: the sets of tcdiff_*, tcx_*, tcs_*, tcr_*, tcj_*, tck_*, tcg_*, tcp_*, tcf_* and tcm_* symbols the
 * library exports are frozen (the tests hold each equal to the built library's dynamic symbols).  This header takes a prefix of its
 * own; tcdiff_amd/_lib.py binds it as SELF next to the others and adds it to none of them nor to EXPORTS.
 *
 * Why it is not a flag of tcg_group_metrics: it looks at one dancer (dn = 1 is legal, dn rows per clip and not dn (dn - 1) / 2); the
 * neighbouring capsules of a body overlap by construction, so it needs a list of the bone pairs that may collide; and "which limbs?"
 * needs an answer per bone pair.
 *
 * The reference has no counterpart.  The metric is the project's own; parity with any other tool is unpinned, and what follows is
 * the definition.  csrc/selfcontact_math.h (with csrc/group_math.h) is its arithmetic, tests/selfcontact_ref.py its numpy
 * restatement.  The capsule radii, the tolerance and the list of bone pairs (tcdiff_amd/self_contact.py builds a default one from
 * `hops` and `rest_margin`) are choices, not measurements.
 * Not built: resolving a self-contact (bending an arm to dodge); mesh-level self-contact (a sub-mesh of one body is not closed, so
 * the winding number of tcdiff_meshcontact.h does not apply); drawing it; any use inside the sampler.
 *
 * ---- input ----------------------------------------------------------------------------------------------------------------------
 * joints: float32, read in place; joint j, component k of (clip c, dancer d, frame t) is at
 * joints + c strides[0] + d strides[1] + t strides[2] + 3 j + k (element strides, each >= 0; the trailing 24 x 3 is contiguous).
 * b >= 1 clips, dn >= 1 dancers, T >= 1 frames; (clip c, dancer d) is row c dn + d of every output.  All arithmetic is float64 on
 * the float32 inputs, every product and sum rounded on its own (no contraction); comparisons are of float64 values.
 *
 * ---- capsules and distance ------------------------------------------------------------------------------------------------------
 * Section 1 of tcdiff_group.h, word for word: bone i = 1 .. 23 is the segment J[parents[i]] -> J[i], a capsule of radius radii[i]
 * (metres; entry 0 is unused); dist of two segments is the clamped closest-point construction stated there (csrc/group_math.h).
 *
 * ---- bone pairs -----------------------------------------------------------------------------------------------------------------
 * The TC_SELF_PAIRS = 253 unordered pairs (i, j), 1 <= i < j <= 23, are numbered k = 0 .. 252 in lexicographic order: (1,2), (1,3),
 * ..., (1,23), (2,3), ..., (22,23).  `mask` is four HOST 64-bit words; pair k is LISTED if bit k % 64 of word k / 64 is set.
 *
 * ---- per frame t of (clip, dancer) ----------------------------------------------------------------------------------------------
 * gap_k = (dist(bone i, bone j) - radii[i]) - radii[j] for every listed k.
 * gap[t] = the minimum of the listed gap_k in the order of tcg_before: a NaN precedes every number, then the smaller value, then the
 * smaller code 24 i + j; closest[t] = that code.  So a NaN joint on a listed bone makes the frame's gap NaN.
 * pen_k[t] = "k is listed and gap_k < -tolerance" (false for a NaN).  The frame is a CONTACT FRAME if gap[t] < -tolerance.
 * tolerance is finite and >= 0 (metres); contact is strictly deeper than the tolerance.
 *
 * ---- per (clip, dancer), over its T frames --------------------------------------------------------------------------------------
 *   self_contact_rate = contact frames / T;  self_contact_episodes = the number of maximal runs of contact frames;
 *   self_gap_min = the smallest FINITE gap[t], NaN if no frame has one;
 *   self_closest = (t, i, j) of that gap, the first such frame on a tie; (-1, -1, -1) if there is none;
 *   self_depth_mean = (the sum of -gap[t] over the contact frames) / their number, NaN if there is none.  The sum is that of
 *     section 3 of tcdiff_group.h: lane l of 64 adds the frames l, l + 64, ... in ascending order starting from 0.0 (skipping the
 *     frames that are no contact frames), then the 64 partial sums are added pairwise with the lane whose number differs in bit 5,
 *     then bit 4, ... bit 0;
 *   self_pair_frames[k] = the number of frames with pen_k[t], k = 0 .. 252; 0 for a pair that is not listed.
 *
 * ---- the launchers (csrc/selfcontact.hip) ---------------------------------------------------------------------------------------
 * TC_SELF_LAUNCHES launches whatever b is, no atomics anywhere, every reduction in a fixed order: the same input gives the same bits.
 * 1. frames: one wave per (clip, dancer, frame), four frames per workgroup of 256 (the frames of a partial last workgroup are masked
 *    off, not computed); the 24 joints staged once in LDS as float64; lane l of round r takes pair k = l + 64 r, four rounds; a pair
 *    that is not listed takes no part in the minimum; a cross-lane minimum of (gap, code) in the total order above; the four 64-bit
 *    ballots of pen_k are the frame's penetration words.  Lane 0 writes the gap and the code (to the caller's `gap` / `closest` if
 *    given, else to the workspace) and the four words (to the workspace).
 * 2. dancers: one workgroup of 256 per (clip, dancer): the gap plane reduced over T (integer counts; the episodes; the finite minimum
 *    with its frame, a tree over tcg_before_finite; the depth sum in the lane order above, by the first wave); pair_frames by thread
 *    k < 253, which tests its bit of every frame's words in ascending t (integers: exact).
 * workspace: TC_SELF_WS_FRAME bytes per (clip, dancer, frame) -- four 8-byte words, a gap, a code -- rounded up to a multiple of 8;
 * aligned to 8.
 *
 * The checks, in this order.  TC_ERR_ARG: a NULL pointer (gap and closest may be NULL); b < 1, dn < 1 or T < 1; a tolerance that is
 * negative or not finite.  TC_ERR_UNSUPPORTED: more than 2^31 - 1 (clip, dancer, frame) triples.  TC_ERR_ARG: a negative stride; a
 * parent of joint 1 .. 23 that is negative or does not precede its child; a radius of bone 1 .. 23 that is negative or not finite; a
 * set bit of `mask` at k >= 253; an empty mask; workspace_bytes below tci_self_contact_workspace's.  TC_ERR_ALIGN: workspace or gap
 * not aligned to 8 bytes, closest not to 4.
 * tci_self_contact_workspace: TC_ERR_ARG for a NULL `bytes`, the same shape checks, TC_ERR_UNSUPPORTED likewise. */
#ifndef TCDIFF_SELFCONTACT_H
#define TCDIFF_SELFCONTACT_H

#include "tcdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TC_SELF_LAUNCHES 2
#define TC_SELF_PAIRS 253
#define TC_SELF_WS_FRAME 44

/* bytes[0] (a HOST long) = the workspace tci_self_contact needs for b clips of dn dancers and T frames */
int tci_self_contact_workspace(int b, int dn, int T, long* bytes);

/* gap [b dn][T] float64 and closest [b dn][T] int32: the per-frame planes, or NULL.  rate, gap_min, depth_mean [b dn] float64;
 * episodes [b dn], closest_min [b dn][3] and pair_frames [b dn][253] int64 (long). */
int tci_self_contact(const float* joints, const long* joint_strides, int b, int dn, int T, const int* parents, const double* radii,
                     const uint64_t* mask, double tolerance, void* workspace, long workspace_bytes, double* gap, int* closest,
                     double* rate, double* gap_min, long* episodes, long* closest_min, double* depth_mean, long* pair_frames,
                     hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TCDIFF_SELFCONTACT_H */
