/* tcdiff_footlock.h -- the seventh header of libtcdiff_gfx950.so's C ABI: the foot lock, a post-process on the exported poses.  While
 * the model declares a foot planted, the foot is held where it stood, and hip and knee are re-solved by analytic two-bone inverse
 * kinematics; the foot keeps its world orientation; the correction is eased in and out around the contact.  The conventions of
 * tcdiff_hip.h hold: every function returns 0 or a negative TC_ERR_* code, nothing is allocated, nothing synchronises the host,
 * pointers are caller-owned DEVICE pointers (`contact_strides`, `parents`, `offsets` and `bytes` excepted: HOST), work is enqueued on
 * `stream`, the checks precede any GPU call.
 *
 * Why the functions are tck_*: the sets of tcdiff_*, tcx_*, tcs_*, tcr_* and tcj_* symbols the library exports are frozen (the tests
 * hold each equal to the built library's dynamic symbols).  This header takes a prefix of its own; tcdiff_amd/_lib.py binds it as
 * FOOTLOCK next to ABI, EXT, GLTF, SKIN, SHADE and MJPEG and adds it to none of them nor to EXPORTS.
 *
 * The reference has no counterpart (it renders the raw poses), so what follows is restated from the textbook construction and is
 * the definition; parity with any other tool is unpinned.  csrc/footlock_math.h is its arithmetic, tests/footlock_ref.py its numpy
 * restatement.  Not built: smoothing the jump of the shift where two runs touch; floor penetration and the height of the anchor;
 * toe-joint articulation; hands; correcting the root; locking inside the sampler; any change to what the sampler or the training
 * loss computes.
 *
 * ---- input ----------------------------------------------------------------------------------------------------------------------
 * q [b][T dn][24][3] float32 rotation vectors and pos [b][T dn][3] float32 root positions, contiguous, row = frame dn + dancer: what
 * tcdiff_pose_export writes (long mode: b = 1).  contacts: NULL, or float32 read in place, element (clip c, dancer d, frame t,
 * channel k) at contacts + c strides[0] + d strides[1] + t strides[2] + k strides[3] (element strides, each >= 0); the channels are
 * the joints 7, 8, 10, 11 in this order (left ankle, right ankle, left toe, right toe).  parents [24], offsets [24][3]: the skeleton
 * of tcdiff_pose_export; the legs must be SMPL's: (hip h, knee k, ankle a, toe e) = (1, 4, 7, 10) on the left, (2, 5, 8, 11) on the
 * right, each joint the child of the one before and the hips children of joint 0.
 *
 * All of the following is per clip, dancer and leg, in float64 arithmetic on the float32 inputs, every product and sum rounded on its
 * own (no contraction), each output component rounded to float32 once, at the store.
 *
 * ---- 1. the chain -------------------------------------------------------------------------------------------------------------------
 * The unit quaternion (w, x, y, z) of a rotation vector r, as csrc/gltf_math.h forms it: theta = sqrt((r0 r0 + r1 r1) + r2 r2),
 * k = sin(theta / 2) / theta, or (1/2 - theta^2 / 48) + theta^4 / 3840 for theta < 1e-3; (cos(theta / 2), k r0, k r1, k r2).
 * The product a (x) b is Hamilton's; R . v = v + w t + u x t with u = (x, y, z), t = 2 (u x v).  No quaternion is renormalised.
 *   R_0 = quat(q_0), P_0 = pos;   for j in h, k, a (p the parent):  P_j = P_p + R_p . off_j,  R_j = R_p (x) quat(q_j);
 *   P_e = P_a + R_a . off_e.      l1 = |off_k|, l2 = |off_a|.
 *
 * ---- 2. labels --------------------------------------------------------------------------------------------------------------------
 * With contacts: c_f[t] = contacts[t, channel of f] > contact_threshold, a float32 compare.  Without (long mode has none):
 * c_f[t] = |P_f[t + 1] - P_f[t]| < still for t < T - 1, and c_f[T - 1] is true -- the dataset's own rule
 * (dataset/group_dataset.py:204-207), on the float64 chain.  The pin joint g[t]: the ankle if c_a[t], else the toe if c_e[t], else
 * none.  A frame with a pin joint is planted.  A run is a maximal interval of frames with the same pin joint; an ankle run and a toe
 * run that touch are two runs.
 *
 * ---- 3. anchor and wanted shift -------------------------------------------------------------------------------------------------------
 * A(run) = (sum of P_g[t] over the run, added in ascending t, starting from the first frame's value added to 0) / the run's frames.
 * In a run d[t] = A - P_g[t]: the foot is translated, so ankle and toe move alike.  Outside the runs let t0 be the nearest planted
 * frame before t and t1 the nearest after (either may be absent), G = t1 - t0:
 *   both exist and G - 1 <= 2 blend:   d[t] = ((t1 - t) d[t0] + (t - t0) d[t1]) / G
 *   otherwise:                         d[t] = lambda(t - t0) d[t0] + lambda(t1 - t) d[t1],  lambda(s) = max(0, 1 - s / (blend + 1)),
 *                                      an absent side contributing 0 (the two ramps cannot overlap here).
 * blend = 0 means no easing.  A frame whose d[t] is zero in all three components copies its nine input floats through, bit for bit.
 * Where two runs touch, d jumps; it is left so (see "not built").
 *
 * ---- 4. the two-bone solve of a frame with d != 0 ---------------------------------------------------------------------------------------
 * H = P_h, K = P_k, A = P_a, v = A - H, r = |v|, v' = (A + d) - H.  If |v'| < 1e-9 the frame is left unchanged.
 * Reach: r_max = (l1 + l2)(1 - reach), r_min = |l1 - l2| + reach (l1 + l2), r' = max(min(|v'|, max(r_max, r)), r_min).  If r' != |v'|
 * the frame counts as clamped, and the ankle goes to H + r' v' / |v'|.
 * Flexion now: a = K - H, b = A - K, theta = atan2(|a x b|, a . b).  Bend axis n = a x b / |a x b|; if
 * |a x b| < 1e-9 l1 l2 (a straight or folded leg), x = R_h . (1, 0, 0), p = x - a ((x . a) / (a . a)), n = p / |p| -- the hip's x axis
 * made perpendicular to the thigh, for an axis that is not perpendicular to the bones changes the flexion by less than the angle it
 * turns by -- and the frame is left unchanged if |p| < 1e-9.
 * Flexion wanted: theta' = pi - acos(clamp(((l1^2 + l2^2) - r'^2) / (2 l1 l2), -1, 1)); the change is theta' - theta, and exactly 0
 * if r' == r.
 * S1 = the rotation about n by that change, (cos(phi / 2), n sin(phi / 2)).  A1 = K + S1 . b.
 * S2 = the shortest arc from u1 = (A1 - H) / |A1 - H| to u2 = v' / |v'|: axis (u1 x u2) / |u1 x u2|, angle atan2(|u1 x u2|, u1 . u2);
 * the identity if |u1 x u2| < 1e-300, unless u1 . u2 < 0 (antiparallel), when the frame is left unchanged.
 * World rotations: R_h' = S2 (x) R_h, R_k' = (S2 (x) S1) (x) R_k, R_a' = R_a -- the foot keeps its world orientation, so the toe's
 * offset from the ankle is unchanged.  Locals: conj(R_0) (x) R_h', conj(R_h') (x) R_k', conj(R_k') (x) R_a.  Each is negated if
 * w < 0, then turned into a rotation vector: theta = 2 atan2(|xyz|, w), xyz / k(theta) with the k of step 1.
 *
 * ---- outputs ----------------------------------------------------------------------------------------------------------------------
 * q_out [b][T dn][24][3]: q with joints 1, 4, 7 and 2, 5, 8 of the solved frames replaced; every other float is the input's word.
 * joints (or NULL) [b][dn][T][24][3]: the float32 FK of q_out and pos by the chain of tcdiff_pose_export (csrc/fk_math.h fk_forward).
 * planted, clamped [b][dn][2] int32: per leg (left, right) the planted frames and the frames counted as clamped by the reach test.
 * max_shift [b][dn][2] float64: per leg the largest |d[t]| over all frames, in metres.  pos is never written.
 *
 * ---- the launchers (csrc/footlock.hip) ------------------------------------------------------------------------------------------------
 * TC_FOOTLOCK_LAUNCHES launches whatever b is.  1. frames: one thread per (clip, dancer, frame) -- the chain down both legs and the
 * labels into the workspace, structure of arrays over the frame slot (clip dn + dancer) T + frame; frame t + 1 of the displacement
 * rule is read and recomputed, not exchanged.  2. runs: one wave per (clip, dancer, leg), lanes over frames in chunks of
 * TC_FOOTLOCK_CHUNK -- run ends from a wave ballot of the label changes, the open run carried across chunks, the anchor sums in
 * ascending t, a backward pass for t1 and a forward pass for t0; writes d[t] and the three diagnostics; no atomics, every reduction
 * in a fixed order: the same input gives the same bits.  3. solve: one thread per (clip, dancer, frame) -- step 4 for both legs, the
 * pose stored, the FK if asked.  workspace: TC_FOOTLOCK_WS_PER_FRAME bytes per (clip, dancer, frame), aligned to 8.
 *
 * The checks, in this order.  TC_ERR_ARG: a NULL pointer (contacts and joints may be NULL; contact_strides may be if contacts is);
 * blend < 0; reach outside (0, 0.5); still < 0 or NaN; a NaN contact_threshold; b, dn or T < 1.  TC_ERR_UNSUPPORTED: more than
 * 2^31 - 1 frame slots or 2^30 - 1 (clip, dancer) pairs; blend above 2^26 - 1.  TC_ERR_ARG: a negative stride; a parent that does not precede its child.
 * TC_ERR_UNSUPPORTED: legs that are not SMPL's; a thigh or shin of length 0 or not finite.  TC_ERR_ARG: workspace_bytes below
 * tck_foot_lock_workspace's.  TC_ERR_ALIGN: workspace not aligned to 8 bytes. */
#ifndef TCDIFF_FOOTLOCK_H
#define TCDIFF_FOOTLOCK_H

#include "tcdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TC_FOOTLOCK_LAUNCHES 3
#define TC_FOOTLOCK_CHUNK 64
#define TC_FOOTLOCK_WS_PER_FRAME 480

/* bytes[0] (a HOST long) = the workspace tck_foot_lock needs for b clips of dn dancers and T frames */
int tck_foot_lock_workspace(int b, int dn, int T, long* bytes);

int tck_foot_lock(const float* q, const float* pos, const float* contacts, const long* contact_strides, int b, int dn, int T,
                  float contact_threshold, double still, int blend, double reach, const int* parents, const float* offsets,
                  void* workspace, long workspace_bytes, float* q_out, float* joints, int* planted, int* clamped,
                  double* max_shift, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TCDIFF_FOOTLOCK_H */
