/* tcdiff_beatsync.h -- the fifteenth header of libtcdiff_gfx950.so's C ABI: WHERE are a dancer's kinematic beats, and a monotone time
 * warp that brings them onto the music's.  beat_align of tcdiff_motion_metrics (tcdiff_hip.h) says in one float per dancer how far the
 * minima of the smoothed joint speed lie from the music's beats; tcb_motion_beats returns the curve and the minima themselves, and
 * tcb_beat_sync retimes the poses that tcdiff_pose_export leaves on the device so that matched minima land on their beats.  The
 * conventions of tcdiff_hip.h hold: every function returns 0 or a negative TC_ERR_* code, nothing is allocated, nothing synchronises the
 * host, nothing is copied to the host, pointers are caller-owned DEVICE pointers (`joint_strides`, `parents`, `offsets` and `bytes`
 * excepted: HOST), work is enqueued on `stream`, the checks precede any GPU call.
 *
 * Why the functions are tcb_*: the sets of tcdiff_*, tcx_*, tcs_*, tcr_*, tcj_*, tck_*, tcg_*, tcp_*, tcf_*, tcm_*, tci_*, tcw_* and
 * tcc_* symbols the library exports are frozen (the tests hold each equal to the built library's dynamic symbols).  This header takes a
 * prefix of its own; tcdiff_amd/_lib.py binds it as BEATSYNC next to the others and adds it to none of them nor to EXPORTS.
 *
 * The reference has no counterpart (it renders the raw poses).  The speed curve is beat_align's own (Bailando's, tcdiff_hip.h); the
 * rest -- nearest-beat matching, the PCHIP warp through the interpolant of tcdiff_choreo.h, slerp resampling -- is the project's own,
 * parity with any other tool is unpinned, and what follows is the definition.  csrc/beatsync_math.h (on csrc/choreo_math.h,
 * csrc/footlock_math.h and csrc/fk_math.h, unchanged) is its arithmetic, tests/beatsync_ref.py its numpy restatement.
 * max_shift = 7, max_rate = 1.5, strength = 1, sigma_smooth = 5, the linear root interpolation and the nearest-frame contacts are
 * choices, not measurements.
 * Not promised: that the smoothed speed minimum of the warped motion lands exactly on its beat (the warp's own rate modulates the
 * speed); that a trajectory error stays (the root path is shifted in time by up to max_shift frames of travel); with separate warps,
 * that the contacts between dancers stay.
 * Not built: snapping choreography keys to beats; retiming inside the sampler; changing the clip length; cubic root interpolation; a
 * musical-phrase or downbeat model; warping cond.
 *
 * All arithmetic is float64 on the float32 inputs, every product and sum rounded on its own (no contraction), every sum in the order
 * written; each float32 output is rounded once, at the store.  Every extremum is over a total order, the lower frame winning a tie.
 * No atomics anywhere: the same input gives the same bits.
 *
 * Shapes.  b >= 1 clips, dn >= 1 dancers, 1 <= T <= TC_BEATSYNC_MAX_FRAMES frames, N = T - 1.  A WARP is the unit that is retimed
 * together: with `share` the dn dancers of a clip share one warp (W = 1), without it every dancer has its own (W = dn); warp w of clip
 * c is row c W + w of every per-warp output, (clip c, dancer d) row c dn + d of every per-dancer output.
 * TC_BEATSYNC_MAX_FRAMES = 4096 bounds the lists launch 2 keeps in LDS (36 T bytes and a little: 144 KiB of the CU's 160 KiB at 4096, 42 KiB
 * for a song of 1200 frames, sized from T at launch).
 *
 * ==== 1. the speed curve and the kinematic beats ======================================================================================
 * J[t][j]: the float32 position of joint j in frame t -- tcb_motion_beats reads it in place: component k of (clip c, dancer d, frame
 * t) is at joints + c strides[0] + d strides[1] + t strides[2] + 3 j + k (element strides, each >= 0; the trailing 24 x 3 is
 * contiguous); tcb_beat_sync forms it as the float32 FK of its INPUT (csrc/fk_math.h fk_forward of q and pos, the chain of
 * tcdiff_pose_export, the joints tcdiff_motion_metrics would be handed).
 *   v_d[t] = (the sum over j = 0 .. 23, in ascending j to 0.0, of sqrt((dx dx + dy dy) + dz dz), d = J[t+1][j] - J[t][j]) / 24, t < N.
 *   The warp's curve pv: v_d itself without `share`; with it (the sum over d = 0 .. dn-1, in ascending d to 0.0, of v_d[t]) / dn.
 *   s[t] = the sum over x = -rad .. rad, in ascending x to 0.0, of weights[x + rad] pv[r(t + x)], r(i) = i mod 2N, mirrored to
 *   2N - 1 - that where it is >= N: scipy.ndimage.gaussian_filter1d(pv, sigma, mode="reflect") as tcdiff_hip.h states it for beat_align.
 *   weights [2 rad + 1] float64 on the DEVICE, built by the caller on the HOST in float64: exp(-0.5 / sigma^2 x^2) over their sum,
 *   rad = int(4 sigma + 0.5) <= TC_BEATSYNC_MAX_RADIUS; the kernel and the restatement multiply the same doubles in the same order.
 *   status = 1 if some pv[t] is not finite, else 0.
 *   kin[t] = 1 if status = 0 and 1 <= t <= N - 2 and s[t] < s[t-1] and s[t] < s[t+1], else 0 (t < T): the strict interior local minima;
 *   T < 4 has none.  kin_count = their number.  speed [b][W][N] = s; with status = 1 every word of it is the quiet NaN
 *   0x7ff8000000000000.
 *
 * ==== 2. matching (tcb_beat_sync) =================================================================================================
 * beats [b][T] uint8.  The music beats of a clip are the frames 0 < m < T - 1 with beats[m] != 0, music_count their number: the end
 * frames are pinned.  Each m picks the kinematic beat k with the smallest |k - m|, of two at the same distance the lower k, if
 * |k - m| <= max_shift; otherwise it is unmatched.  A k picked by several m keeps the one with the smallest |k - m|, of two at the same
 * distance the lower m; the others are unmatched and do not look for a second choice.  `matched` = the pairs (m, k) that remain,
 * the CANDIDATES, in ascending m (their k ascend as well).  With status = 1 there are none.
 *
 * ==== 3. anchors ================================================================================================================
 * The shift of a candidate is e = strength (k - m), its source time u = m + e (the product rounded, then the sum).  lo = 1 / max_rate.
 * Start from the fixed anchor (m0, u0) = (0, 0) and go through the candidates in ascending m: with r = (u - u0) / (m - m0) against
 * the last accepted anchor, accept (m, u) if lo <= r <= max_rate, otherwise dropped += 1.  Then close with the fixed anchor
 * (T - 1, T - 1): while a candidate is kept and r = ((T - 1) - u) / ((T - 1) - m) of the last kept one lies outside [lo, max_rate], pop it and
 * dropped += 1.  `anchors` = the candidates kept.  This is one lane's serial pass over at most T / 2 items.
 *
 * ==== 4. the warp ===============================================================================================================
 * warp [b][W][T] float64: the source time of every output frame.  With no candidate kept (and with status = 1) warp[t] = t exactly.
 * Otherwise the keys are 0, the kept m and T - 1, the values 0, the kept u and T - 1 in float64, and the slopes D those of PCHIP
 * (tcc_slope of csrc/choreo_math.h, Fritsch-Butland, as tcdiff_choreo.h states them): ascending values give a nondecreasing cubic.
 * That cubic is evaluated about the diagonal -- a Hermite form is linear in its values and slopes, and the one through (m, m) with
 * slopes 1 is t itself --: warp[t] = t + tcc_eval(keys, the shifts 0, e, .., 0, the slopes D - 1, t), the sum rounded once, then
 * clamped to [0, T - 1].  So a key frame is m + e = u bit for bit, and anchors on the diagonal (strength = 0) give warp[t] = t exactly.
 *   shift_max = the largest |warp[t] - t| (0 without a frame that moves).
 *   rate_min, rate_max = the smallest and the largest warp[t+1] - warp[t], t < N, with rate_min_frame, rate_max_frame (the lower frame
 *   on a tie); T = 1: NaN and -1.
 *
 * ==== 5. resampling, per (clip, dancer, output frame t) ==============================================================================
 * q [b][T dn][24][3] float32 rotation vectors, pos [b][T dn][3] float32 root positions, row = frame dn + dancer: what
 * tcdiff_pose_export writes (long mode: b = 1); contacts (or NULL) [b][dn][T][4] float32.  Outputs of the same shapes.
 * u = warp[t] of the dancer's warp, i = floor(u), a = u - i.  (u <= T - 1, so i = T - 1 only with a = 0: the last frame is copied, never
 * extrapolated; where a != 0, i <= T - 2.)
 *   a == 0: every output float of the frame (rotations, root, contacts) is source frame i's word.
 *   otherwise
 *     the root: ((1 - a) p[i][c] + a p[i+1][c]) per component, rounded once.  If one of the six floats is not finite the three floats
 *       of pos[t] are copied through bit for bit and copied += 1.
 *     joint j: A = tck_quat(q[i][j]), B = tck_quat(q[i+1][j]) (csrc/footlock_math.h, the conversion of tcdiff_smooth.h);
 *       d = ((A.w B.w + A.x B.x) + A.y B.y) + A.z B.z; if d < 0, d = -d and B = -B (the first's hemisphere); if 1 - d < 0.01 the
 *       weights are (1 - a, a) (the linear fallback of stitch.quat_slerp), else with om = acos(d): sin((1 - a) om) / sin(om) and
 *       sin(a om) / sin(om); R = w0 A + w1 B per component; n = sqrt(((R.w^2 + R.x^2) + R.y^2) + R.z^2); q_out[t][j] =
 *       tck_rotvec(R / n), rounded once.  If one of the six floats is not finite the three floats of q[t][j] are copied through
 *       bit for bit and copied += 1.
 *     contacts: the four words of source frame i if a < 0.5, else of i + 1, bit for bit.
 *   moved [b dn] = the frames with warp[t] != t; copied [b dn] as counted above; both int32.
 *   joints [b][dn][T][24][3] float32: fk_forward of q_out and pos_out; joints_in (or NULL): the same of q and pos (the J of section 1).
 *
 * ==== the launchers (csrc/beatsync.hip), TC_BEATSYNC_LAUNCHES launches whatever the number of clips ======================================
 * 1. one workgroup of 64 per (clip, dancer, tile of TC_BEATSYNC_TILE - 1 frames): lane l runs fk_forward of frame t0 + l into LDS (and
 *    joints_in), then forms v of its frame from its own and the next lane's joints, and the frame's non-finite mask (a bit per joint,
 *    bit 24 the root) -- both into the workspace.  tcb_motion_beats: a thread per (clip, dancer, frame) reads the joints in place.
 * 2. one workgroup of 256 per warp: pv into LDS, status, s (LDS and `speed`), the minima; the kinematic and the music beats compacted
 *    into LDS lists by ballot and prefix; a lane per music beat for the nearest kinematic beat (binary search) and for whether it
 *    keeps its claim; the candidates compacted; the serial anchor pass on lane 0; a lane per anchor for the slopes; a thread per
 *    frame for warp; the reductions (integers and maxima of numbers: order-free; the rates: a tree over the total order), among
 *    them moved and copied of the warp's dancers from launch 1's masks.  tcb_motion_beats stops after the minima.
 * 3. one workgroup of 256 per (clip, dancer, tile of TC_BEATSYNC_TILE frames): the 24 slerps and the root of the tile's frames over
 *    the threads into LDS and q_out / pos_out / contacts_out, then lane l of the first wave runs fk_forward of frame t0 + l.
 * workspace: per (clip, dancer, frame) one float64 (v) and one int32 (the mask); aligned to 8.
 *
 * The checks, in this order.  TC_ERR_ARG: a NULL pointer (contacts with contacts_out, and joints_in, may be NULL; contacts without
 * contacts_out or the reverse is an error); b, dn or T < 1; share not 0 or 1; rad < 0; max_shift < 0; max_rate not in [1, 1e6];
 * strength not in [0, 1].  TC_ERR_UNSUPPORTED: T > TC_BEATSYNC_MAX_FRAMES; rad > TC_BEATSYNC_MAX_RADIUS; more than 2^31 - 1 (clip,
 * dancer, frame) triples.  TC_ERR_ARG: a negative stride (tcb_motion_beats); a parent that does not precede its child (tcb_beat_sync);
 * workspace_bytes below tcb_beat_sync_workspace's.  TC_ERR_ALIGN: workspace, weights or a float64 output not aligned to 8 bytes, an
 * int32 output not to 4.  tcb_beat_sync_workspace: TC_ERR_ARG for a NULL `bytes`, the same shape checks, TC_ERR_UNSUPPORTED likewise. */
#ifndef TCDIFF_BEATSYNC_H
#define TCDIFF_BEATSYNC_H

#include "tcdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TC_BEATSYNC_LAUNCHES 3
#define TC_BEATSYNC_TILE 64
#define TC_BEATSYNC_MAX_FRAMES 4096
#define TC_BEATSYNC_MAX_RADIUS 512
#define TC_BEATSYNC_WS_FRAME 12

/* bytes[0] (a HOST long) = the workspace tcb_motion_beats and tcb_beat_sync need for b clips of dn dancers and T frames */
int tcb_beat_sync_workspace(int b, int dn, int T, long* bytes);

/* speed [b][W][T - 1] float64, kin [b][W][T] uint8, kin_count [b W] int32; two launches */
int tcb_motion_beats(const float* joints, const long* joint_strides, int b, int dn, int T, int share, int rad, const double* weights,
                     void* workspace, long workspace_bytes, double* speed, unsigned char* kin, int* kin_count, hipStream_t stream);

/* per warp: warp [b][W][T], speed [b][W][T - 1], shift_max, rate_min, rate_max float64; kin [b][W][T] uint8; status, kin_count,
 * music_count, matched, dropped, anchors, rate_min_frame, rate_max_frame int32.  Per (clip, dancer): moved, copied int32. */
int tcb_beat_sync(const float* q, const float* pos, const float* contacts, const unsigned char* beats, int b, int dn, int T, int share,
                  int max_shift, double max_rate, double strength, int rad, const double* weights, const int* parents,
                  const float* offsets, void* workspace, long workspace_bytes, float* q_out, float* pos_out, float* contacts_out,
                  float* joints, float* joints_in, double* warp, double* speed, unsigned char* kin, int* status, int* kin_count,
                  int* music_count, int* matched, int* dropped, int* anchors, double* shift_max, double* rate_min, double* rate_max,
                  int* rate_min_frame, int* rate_max_frame, int* moved, int* copied, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TCDIFF_BEATSYNC_H */
