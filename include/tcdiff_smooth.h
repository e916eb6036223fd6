/* tcdiff_smooth.h -- the thirteenth header of libtcdiff_gfx950.so's C ABI: does a dancer TREMBLE, and a filter against it.  A diffusion
 * sampler predicts its frames as independent rows, and what it returns jitters from frame to frame in the rotations and the root.
 * tcw_smoothness scores that from the joint positions that tcdiff_pose_export (or tck_foot_lock, tcp_keep_apart, tcf_ground,
 * tcw_smooth) leaves on the device; tcw_smooth is a Savitzky-Golay filter of the exported poses, on the root positions and, through
 * unit quaternions, on the rotations.  The conventions of tcdiff_hip.h hold: every function returns 0 or a negative TC_ERR_* code,
 * nothing is allocated, nothing synchronises the host, pointers are caller-owned DEVICE pointers (`joint_strides`, `parents`,
 * `offsets` and `bytes` excepted: HOST), work is enqueued on `stream`, the checks precede any GPU call.
 *
 * Why the functions are tcw_*: the sets of tcdiff_*, tcx_*, tcs_*, tcr_*, tcj_*, tck_*, tcg_*, tcp_*, tcf_*, tcm_* and tci_* symbols
 * the library exports are frozen (the tests hold each equal to the built library's dynamic symbols).  This header takes a prefix of
 * its own; tcdiff_amd/_lib.py binds it as SMOOTH next to the others and adds it to none of them nor to EXPORTS.
 *
 * The reference smooths on the host, per channel (TrajDecoder/utils/utils_model.py:79-86, scipy's savgol_filter with window 21 and
 * order 3); the taps here are those of savgol_filter(..., mode="interp") and are held to scipy on the CPU, the rest -- the quaternion
 * form, the sign rule, the scores -- is the project's own, parity with any other tool is unpinned, and what follows is the
 * definition.  csrc/smooth_math.h (with csrc/footlock_math.h and csrc/fk_math.h, unchanged) is its arithmetic, tests/smooth_ref.py
 * its numpy restatement.  The window and the order are choices, not measurements.
 * Not built: contact-aware taps; a filter inside the sampler; a one-euro or Kalman filter; frequency-domain scores; smoothing the
 * kinks that the correctors' linear envelopes (tck_foot_lock, tcp_keep_apart, tcf_ground) add after it.
 *
 * All arithmetic is float64 on the float32 inputs, every product and sum rounded on its own (no contraction), every sum in the order
 * written; each float32 output is rounded once, at the store.  No atomics anywhere: the same input gives the same bits.
 *
 * ==== 1. tcw_smoothness (one launch) ================================================================================================
 * joints: float32, read in place; joint j, component k of (clip c, dancer d, frame t) is at
 * joints + c strides[0] + d strides[1] + t strides[2] + 3 j + k (element strides, each >= 0; the trailing 24 x 3 is contiguous).
 * b >= 1 clips, dn >= 1 dancers, T >= 4 frames; (clip c, dancer d) is row c dn + d of every output.  fps in (0, 1e6].
 * With p[t] the position of joint j in frame t, |v| = sqrt((v0 v0 + v1 v1) + v2 v2), f2 = fps fps and f3 = f2 fps:
 *   a[t][j] = |(p[t+1] - 2 p[t]) + p[t-1]| f2                        for t = 1 .. T-2   (m/s^2)
 *   k[t][j] = |((p[t+2] - 3 p[t+1]) + 3 p[t]) - p[t-1]| f3           for t = 1 .. T-3   (m/s^3)
 *   kl[t][j] = k of the root-relative positions p_j[t] - p_0[t]      for j = 1 .. 23
 * A term whose value is not finite -- that is, one with a non-finite input -- is left out and is counted out of its mean.
 * The order of every sum: a frame's terms are added in ascending joint order to 0.0; lane l of 64 adds the sums of the frames
 * t = l, l + 64, ... in ascending t to 0.0; the 64 lane sums are added in ascending lane order to 0.0.
 *   accel_mean = sum of a / the terms counted;  jitter = sum of k / the terms counted, `terms` that count;
 *   jitter_local = the same of kl;  root_jitter = the same of k[t][0];  a mean over nothing is NaN.
 *   accel_max, jitter_max: the largest a and k; accel_peak, jitter_peak [2] = its (frame, joint).  The maximum is over a total order:
 *   the larger value, then the lower frame, then the lower joint.  Without a term: NaN and (-1, -1).
 * The launch: one workgroup of 256 per (clip, dancer), 64 frames at a time: every thread forms the terms of six (frame, joint) pairs
 * into LDS, then lane l of the first wave adds the terms of frame l of the 64 in joint order and the frame's sum to its lane sum;
 * lane 0 adds the lane sums; the maxima are a tree over the total order.
 * The checks, in this order.  TC_ERR_ARG: a NULL pointer; b < 1, dn < 1 or T < 4; fps outside (0, 1e6].  TC_ERR_UNSUPPORTED: more than
 * 2^31 - 1 (clip, dancer, frame) triples.  TC_ERR_ARG: a negative stride.  TC_ERR_ALIGN: a float64 output not aligned to 8 bytes, an
 * int32 output not to 4.
 *
 * ==== 2. tcw_smooth (TC_SMOOTH_LAUNCHES launches) ===================================================================================
 * q [b][T dn][24][3] float32 rotation vectors and pos [b][T dn][3] float32 root positions, contiguous, row = frame dn + dancer: what
 * tcdiff_pose_export writes (long mode: b = 1).
 *
 * ---- the tap tables ----------------------------------------------------------------------------------------------------------------
 * taps [W][W] and root_taps [Wr][Wr] float64, on the DEVICE, built by the caller on the host: for an odd window W, 3 <= W <=
 * TC_SMOOTH_MAX_WINDOW, and an order p < W let A be the W x (p + 1) Vandermonde matrix of the offsets -R .. R, R = (W - 1) / 2;
 * the table is A pinv(A).  Row R holds the interior taps; row i < R gives the fitted value at position i of the first W frames, row
 * i > R that of the last W frames: scipy's savgol_filter(..., mode="interp").  T >= W and T >= Wr.
 * Frame t reads the W frames from s = min(max(t - R, 0), T - W) on and uses row t - s: row t over the frames 0 .. W-1 if t < R, row
 * W - (T - t) over T-W .. T-1 if t >= T - R, else row R over t-R .. t+R.  The output frame always lies in its window.
 *
 * ---- the root ----------------------------------------------------------------------------------------------------------------------
 * pos_out[t][c] = the sum over the window (Wr, root_taps), in ascending frame order to 0.0, of tap pos[u][c].  If one of the 3 Wr
 * floats of the window is not finite, the three floats of pos[t] are copied through bit for bit.
 *
 * ---- the rotations, per joint j whose bit of `joints_mask` is set ------------------------------------------------------------------
 * Q[u] = the unit quaternion of q[u][j] (tck_quat of csrc/footlock_math.h).  s[u] = -1 if ((Q[t].w Q[u].w + Q[t].x Q[u].x) +
 * Q[t].y Q[u].y) + Q[t].z Q[u].z < 0, else +1.  acc = the sum over the window, in ascending frame order to 0.0 per component, of
 * (tap s[u]) Q[u].  n = sqrt(((acc.w^2 + acc.x^2) + acc.y^2) + acc.z^2).  If n >= 1e-6: q_out[t][j] = tck_rotvec(acc / n) -- a
 * linear filter in R^4 projected back to the unit sphere, the chordal mean generalised to signed taps; it never averages q with -q.
 * Otherwise -- n < 1e-6, or a non-finite float of joint j in the window, which makes n NaN -- the joint's three floats are copied
 * through bit for bit.  A joint whose bit is clear is copied through as well.
 *
 * ---- outputs -----------------------------------------------------------------------------------------------------------------------
 * q_out, pos_out: as q and pos.  joints (or NULL) [b][dn][T][24][3]: the float32 FK of q_out and pos_out by the chain of
 * tcdiff_pose_export (csrc/fk_math.h fk_forward), the layout of tck_foot_lock's joints.  joints_in (or NULL): the same of q and pos.
 * Per (clip, dancer), row c dn + d:
 *   max_rot_change float64: the largest finite 2 atan2(|xyz|, |w|) of conj(tck_quat(q[t][j])) (x) tck_quat(q_out[t][j]) over all
 *     frames and joints, of the float32 values as stored, in radians; 0 if there is none.
 *   max_pos_change float64: the largest finite |pos_out[t] - pos[t]|, likewise, in metres.
 *   copied int32: the outputs copied through for want of a finite or non-degenerate window: one per (frame, joint with its bit set)
 *     and one per frame's root.  The joints whose bit is clear are not counted.
 *
 * ---- the launchers (csrc/smooth.hip) -----------------------------------------------------------------------------------------------
 * 1. filter: one workgroup of 256 per (clip, dancer, tile of TC_SMOOTH_TILE frames).  The quaternions of the tile's frames and their
 *    halo (for the edge tiles: the first or last W frames) are formed once and staged in LDS as float64, 24 x 4 component rows of
 *    64 + W - 1 frames each: 54 KiB at W = 9, 94.5 KiB at W = 63 of the CU's 160 KiB, sized from W at launch.  A
 *    row holds ONE component of one joint over the frames, so the 64 lanes that filter one joint's consecutive frames read
 *    consecutive words.  The root's three rows are staged likewise.  Then wave w takes the joints w, w + 4, ..., lane l the tile's
 *    frame l: the tap loop in ascending order, q_out stored, the change of what was stored measured; the first wave does the root.
 *    The tile's largest rotation change, largest root change and copied outputs go to the workspace.
 * 2. FK and stats: one thread per (clip, dancer, frame) runs fk_forward of the output, as many again that of the input if asked;
 *    trailing blocks, a thread per (clip, dancer), reduce the tiles of launch 1 in ascending order (maxima and integers: order-free).
 *    They read nothing that launch 2 writes.
 * workspace: TC_SMOOTH_WS_TILE bytes per (clip, dancer, tile) -- two float64 and an int32 -- rounded up to a multiple of 8; aligned
 * to 8.
 *
 * The checks, in this order.  TC_ERR_ARG: a NULL pointer (joints and joints_in may be NULL); b, dn or T < 1; window or root_window
 * even or outside 3 .. TC_SMOOTH_MAX_WINDOW; T < window or T < root_window; a bit of joints_mask at 24 or above.
 * TC_ERR_UNSUPPORTED: more than 2^31 - 1 frame slots.  TC_ERR_ARG: a parent that does not precede its child; workspace_bytes below
 * tcw_smooth_workspace's.  TC_ERR_ALIGN: workspace, taps, root_taps, max_rot_change or max_pos_change not aligned to 8 bytes.
 * tcw_smooth_workspace: TC_ERR_ARG for a NULL `bytes`, the same shape checks, TC_ERR_UNSUPPORTED likewise. */
#ifndef TCDIFF_SMOOTH_H
#define TCDIFF_SMOOTH_H

#include "tcdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TC_SMOOTH_LAUNCHES 2
#define TC_SMOOTH_TILE 64
#define TC_SMOOTH_MAX_WINDOW 63
#define TC_SMOOTH_WS_TILE 20

/* accel_mean, jitter, jitter_local, root_jitter, accel_max, jitter_max [b dn] float64; accel_peak, jitter_peak [b dn][2] and terms
 * [b dn] int32 */
int tcw_smoothness(const float* joints, const long* joint_strides, int b, int dn, int T, double fps, double* accel_mean, double* jitter,
                   double* jitter_local, double* root_jitter, double* accel_max, double* jitter_max, int* accel_peak, int* jitter_peak,
                   int* terms, hipStream_t stream);

/* bytes[0] (a HOST long) = the workspace tcw_smooth needs for b clips of dn dancers and T frames */
int tcw_smooth_workspace(int b, int dn, int T, long* bytes);

int tcw_smooth(const float* q, const float* pos, int b, int dn, int T, int window, const double* taps, int root_window,
               const double* root_taps, unsigned joints_mask, const int* parents, const float* offsets, void* workspace,
               long workspace_bytes, float* q_out, float* pos_out, float* joints, float* joints_in, double* max_rot_change,
               double* max_pos_change, int* copied, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TCDIFF_SMOOTH_H */
