/* tcdiff_group.h -- the eighth header of libtcdiff_gfx950.so's C ABI: scores of the GROUP, computed from the joint positions that
 * tcdiff_pose_export (or tck_foot_lock) leaves on the device.  Three questions per clip and pair of dancers: do the bodies touch, do
 * the dancers walk through each other's paths, do they move together.  The conventions of tcdiff_hip.h hold: every function returns
 * 0 or a negative TC_ERR_* code, nothing is allocated, nothing synchronises the host, pointers are caller-owned DEVICE pointers
 * (`joint_strides`, `parents`, `radii` and `bytes` excepted: HOST), work is enqueued on `stream`, the checks precede any GPU call.
 *
 * Why the functions are tcg_*: the sets of tcdiff_*, tcx_*, tcs_*, tcr_*, tcj_* and tck_* symbols the library exports are frozen
 * (the tests hold each equal to the built library's dynamic symbols).  This header takes a prefix of its own; tcdiff_amd/_lib.py
 * binds it as GROUP next to ABI, EXT, GLTF, SKIN, SHADE, MJPEG and FOOTLOCK and adds it to none of them nor to EXPORTS.
 *
 * These metrics are the project's own, in the spirit of AIOZ-GDance's trajectory intersection frequency (TIF) and group motion
 * correlation (GMC); the exact definitions of those are not available to this project, so parity with AIOZ-GDance's code is
 * unpinned, and what follows is the definition.  csrc/group_math.h is its arithmetic, tests/group_ref.py its numpy restatement.
 * The capsule radii, the crossing window, the lag range and sigma_floor are choices, not measurements.
 * Not built: GMR (group motion realism: it needs a trained feature extractor); contact between parts of one dancer; mesh-level
 * penetration from the skinned vertices of tcs_skin_vertices; resolving a contact; drawing it.
 *
 * ---- input ----------------------------------------------------------------------------------------------------------------------
 * joints: float32, read in place; joint j, component k of (clip c, dancer d, frame t) is at
 * joints + c strides[0] + d strides[1] + t strides[2] + 3 j + k (element strides, each >= 0; the trailing 24 x 3 is contiguous).
 * Pairs (a, b), a < b, in lexicographic order: (0,1), (0,2), ..., (1,2), ...; P = dn (dn - 1) / 2; pair p of clip c is row c P + p
 * of every output.  All arithmetic is float64 on the float32 inputs, every product and sum rounded on its own (no contraction);
 * comparisons are of float64 values.  dot(a, b) = (a0 b0 + a1 b1) + a2 b2; |a| = sqrt(dot(a, a)); clamp(x) = 0 if x < 0, 1 if
 * x > 1, else x (a NaN passes through).
 *
 * ---- 1. body gap ------------------------------------------------------------------------------------------------------------------
 * Bone i = 1 .. 23 of a dancer is the segment J[parents[i]] -> J[i], a capsule of radius radii[i] (metres; entry 0 is unused).
 * For pair (a, b) and frame t:  gap[t] = min over (i, j) of dist(bone i of a, bone j of b) - radii[i] - radii[j], evaluated as
 * (dist - radii[i]) - radii[j]; closest[t] = 24 i + j of the minimum, the smallest code on a tie.  A NaN value precedes every number
 * in that order (smallest code among NaNs), so a NaN joint makes the frame's gap NaN.
 * dist of the segments p1 + s d1 and p2 + u d2 (d = end - start), s, u in [0, 1], by the clamped closest-point construction:
 *   r = p1 - p2, A = dot(d1, d1), E = dot(d2, d2), F = dot(d2, r), C = dot(d1, r), B = dot(d1, d2); "small" means <= 1e-18.
 *   A and E small: s = u = 0.     A small: s = 0, u = clamp(F / E).     E small: u = 0, s = clamp(-C / A).
 *   otherwise: den = A E - B B;  s = clamp((B F - C E) / den) if den > 0, else 0;  u = (B s + F) / E;
 *              if u < 0: u = 0, s = clamp(-C / A);   else if u > 1: u = 1, s = clamp((B - C) / A).
 *   dist = |(p1 + s d1) - (p2 + u d2)|, each point formed component by component as p + s d.
 * Over the frames of a pair (T of them): a frame is in contact if gap[t] < 0 (a gap that is not finite is no contact).
 *   body_contact_rate = contact frames / T;  body_contact_episodes = the maximal runs of contact frames;
 *   body_gap_min = the smallest FINITE gap (negative: the penetration depth), NaN if no frame has one;
 *   body_closest = (t, i, j) of that gap, the first such frame on a tie; (-1, -1, -1) if there is none.
 *
 * ---- 2. path crossings ----------------------------------------------------------------------------------------------------------------
 * p_d[t] = the root joint J[t, 0] without its `up` component, the two others in axis order.  Step t of dancer d, t < T - 1, is the
 * floor segment p_d[t] -> p_d[t + 1].  orient(x, y, z) = (y0 - x0)(z1 - x1) - (y1 - x1)(z0 - x0).  Step t of a (a0 -> a1) and
 * step s of b (b0 -> b1) cross when orient(a0, a1, b0) orient(a0, a1, b1) < 0 and orient(b0, b1, a0) orient(b0, b1, a1) < 0: only
 * proper crossings count; a standing dancer or a touching end point is none, nor is anything NaN.
 *   path_crossings = the number of (t, s), 0 <= t, s < T - 1, |s - t| <= window, that cross;
 *   path_crossing_rate = path_crossings / (T - 1), 0 for T < 2.
 * window = 0 asks whether the dancers swap places within one frame; one second of frames asks whether one walks through where the
 * other just was or is about to be.
 *
 * ---- 3. synchrony -----------------------------------------------------------------------------------------------------------------------
 * N = T - 1.  The speed signals, for t < N:  x_d,0[t] = |J[t + 1, 0] - J[t, 0]|;  for j >= 1
 * x_d,j[t] = |(J[t + 1, j] - J[t + 1, 0]) - (J[t, j] - J[t, 0])| -- root-relative, so that travelling in formation does not swamp
 * the limbs.  mu = (sum of x) / N;  sigma = sqrt((sum of (x - mu)^2) / N), the population deviation;  z[t] = (x[t] - mu) / sigma.
 * Both sums: lane l of 64 adds the elements l, l + 64, ... in ascending order starting from 0.0, then the 64 partial sums are
 * added pairwise with the lane whose number differs in bit 5, then bit 4, ... bit 0.
 * Joint j takes part for the pair if sigma_a,j > sigma_floor and sigma_b,j > sigma_floor (false for a NaN).
 *   rho_j(l) = (sum over t of z_a,j[t] z_b,j[t + l], ascending t, both indices in [0, N), starting from 0.0) / (N - |l|)
 *   R(l) = (sum of rho_j(l) over the participating joints, ascending j, starting from 0.0) / their number
 * for the lags |l| <= max_lag with N - |l| >= 2.  sync = max over l of R(l); sync_lag = its l, on a tie the smaller |l|, then the
 * negative one; a positive lag means that b trails a.  sync_zero = R(0).  If no joint takes part or T < 3: NaN, NaN and lag 0.
 *
 * ---- the launchers (csrc/group.hip) ---------------------------------------------------------------------------------------------------
 * TC_GROUP_LAUNCHES launches whatever b is, no atomics anywhere, every reduction in a fixed order: the same input gives the same bits.
 * 1. gap: one wave per (clip, pair, frame), four frames per workgroup of 256; the two dancers' joints staged in LDS as float64;
 *    lane k of round r takes k' = k + 64 r < 529, bone pair (1 + k' / 23, 1 + k' % 23); a cross-lane minimum of (gap, code) in the
 *    total order above; writes the gap / closest planes [b P][T] (the caller's `gap` / `closest` if given, else the workspace's).
 * 2. signals: one workgroup per (clip, dancer): the 24 speeds of every frame, then one wave per joint (six joints each) for mu and
 *    sigma and the standardisation; writes z [b dn][24][T] and sigma [b dn][24] to the workspace.  Standardising here, once per
 *    dancer, keeps the divisions out of the correlation loop.
 * 3. pairs: one workgroup of 256 per (clip, pair): the gap plane reduced over T (integer counts; the minimum with its frame, a tree
 *    over a total order); crossings, a thread per step t looping over s, integer sums; the correlations, items (joint, lag) over
 *    the threads, each summing in ascending t; R and the best lag by one thread in ascending lag.
 * workspace: TC_GROUP_WS_PAIR_FRAME bytes per (clip, pair, frame), TC_GROUP_WS_DANCER_FRAME per (clip, dancer, frame) and
 * TC_GROUP_WS_DANCER per (clip, dancer), rounded up to a multiple of 8; aligned to 8.  max_lag does not change it.
 * fps is checked and otherwise unused: every rate is per frame (tcdiff_amd/group_metrics.py takes its default window from it).
 *
 * The checks, in this order.  TC_ERR_ARG: a NULL pointer (gap and closest may be NULL); b < 1, dn < 2 or T < 1; up outside 0..2;
 * fps not above 0; window < 0; max_lag outside [0, TC_GROUP_MAX_LAG]; sigma_floor negative or NaN.  TC_ERR_UNSUPPORTED: more than
 * 2^31 - 1 (clip, pair, frame) triples or (clip, dancer, joint, frame) values.  TC_ERR_ARG: a negative stride; a parent of joint
 * 1 .. 23 that is negative or does not precede its child; a radius of bone 1 .. 23 that is negative or not finite;
 * workspace_bytes below tcg_group_workspace's.  TC_ERR_ALIGN: workspace or gap not aligned to 8 bytes, closest not to 4.
 * tcg_group_workspace: TC_ERR_ARG for a NULL `bytes`, the same shape and max_lag checks, TC_ERR_UNSUPPORTED likewise. */
#ifndef TCDIFF_GROUP_H
#define TCDIFF_GROUP_H

#include "tcdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TC_GROUP_LAUNCHES 3
#define TC_GROUP_MAX_LAG 64
#define TC_GROUP_WS_PAIR_FRAME 12
#define TC_GROUP_WS_DANCER_FRAME 192
#define TC_GROUP_WS_DANCER 192

/* bytes[0] (a HOST long) = the workspace tcg_group_metrics needs for b clips of dn dancers and T frames */
int tcg_group_workspace(int b, int dn, int T, int max_lag, long* bytes);

/* gap [b P][T] float64 and closest [b P][T] int32: the per-frame planes, or NULL.  contact_rate, gap_min, crossing_rate, sync,
 * sync_zero [b P] float64; episodes, crossings, sync_lag [b P] and closest_min [b P][3] int64 (long). */
int tcg_group_metrics(const float* joints, const long* joint_strides, int b, int dn, int T, int up, double fps,
                      const int* parents, const double* radii, int window, int max_lag, double sigma_floor,
                      void* workspace, long workspace_bytes, double* gap, int* closest,
                      double* contact_rate, double* gap_min, long* episodes, long* closest_min,
                      long* crossings, double* crossing_rate, double* sync, long* sync_lag, double* sync_zero,
                      hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TCDIFF_GROUP_H */
