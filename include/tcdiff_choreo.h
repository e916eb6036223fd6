/* tcdiff_choreo.h -- the fourteenth header of libtcdiff_gfx950.so's C ABI: say WHERE the dancers go, and check that they went there.
 * The model is a trajectory-controllable diffusion: every sampler takes x_0, the floor path of each dancer, and in-paints it into
 * channels 4 and 5.  tcc_plan goes from waypoints in metres ("line at 0 s, circle at 4 s") to that tensor and reports what is wrong
 * with the plan; tcc_trajectory_error measures, after sampling, how far each dancer's root is from the path it was given.  The
 * conventions of tcdiff_hip.h hold: every function returns 0 or a negative TC_ERR_* code, nothing is allocated, nothing synchronises
 * the host, pointers are caller-owned DEVICE pointers (`joint_strides`, `scale` and `min_` excepted: HOST), work is enqueued on
 * `stream`, the checks precede any GPU call.
 *
 * Why the functions are tcc_*: the sets of tcdiff_*, tcx_*, tcs_*, tcr_*, tcj_*, tck_*, tcg_*, tcp_*, tcf_*, tcm_*, tci_* and tcw_*
 * symbols the library exports are frozen (the tests hold each equal to the built library's dynamic symbols).  This header takes a
 * prefix of its own; tcdiff_amd/_lib.py binds it as CHOREO next to the others and adds it to none of them nor to EXPORTS.
 *
 * The reference has no counterpart: its given_trajectory_generation_loop only replays dataset trajectories.  The interpolant is
 * PCHIP (Fritsch-Carlson, with the Fritsch-Butland slopes), restated here as scipy's PchipInterpolator evaluates it and held to it
 * on the CPU; parity with any tool but scipy's interpolator is unpinned, and what follows is the definition.  csrc/choreo_math.h is
 * its arithmetic, tests/choreo_ref.py its numpy restatement.  PCHIP because a choreography HOLDS formations: two equal consecutive
 * waypoints give a dancer who stands still, and a move does not overshoot its target; a natural or Catmull-Rom spline does neither.
 * min_distance and max_speed are choices, not measurements: they only set what the counts too_close and too_fast count.
 * Not built: moving planned paths apart where they come too close (the report only says so; tcp_keep_apart acts after sampling);
 * snapping keys to the beat track; facing direction; per-dancer height; drawing the plan; waypoints at fractional frames; other
 * interpolants.
 *
 * All arithmetic is float64 on the float32 and int32 inputs, every product and sum rounded on its own (no contraction), every sum in
 * the order written; each float32 output is rounded once, at the store.  No atomics anywhere: the same input gives the same bits.
 *
 * ==== 1. tcc_plan (TC_CHOREO_LAUNCHES launches; one when dn = 1) =======================================================================
 * points [b][dn][K][2] float32, contiguous: floor positions in metres, x and y of the data's Z-up frame (that of tcdiff_pose_export's
 * pos).  keys int32: the frames at which they hold, [K] for all dancers (keys_per_dancer = 0) or [b][dn][K].  counts (or NULL: K)
 * [b][dn] int32: how many of the K one dancer uses; what lies beyond is padding and is never read.  1 <= K <= TC_CHOREO_MAX_KEYS,
 * frames >= 1, fps in (0, 1e6].  (clip c, dancer d) is row c dn + d of every per-dancer output.
 *
 * ---- status, decided in the kernel ---------------------------------------------------------------------------------------------------
 *   1: count outside 1 .. K, a key outside [0, frames), or a key not above the one before it;   2 (if not 1): a point that is not
 *   finite;   0 otherwise.  With a status other than 0 the dancer's traj and channels 0 and 1 of its x_0 rows are NaN (channel 2 is
 *   0), clamped and too_fast are 0, speed_peak is -1, speed_max and path_length are NaN.
 *
 * ---- the path, per component y of a dancer with n = count keys -----------------------------------------------------------------------
 * h[k] = key[k+1] - key[k] and m[k] = (y[k+1] - y[k]) / h[k] for k = 0 .. n-2; sign(v) is -1, 0 or 1.
 *   n = 1: the dancer stands at y[0].   n = 2: d[0] = d[1] = m[0], a straight line.   n >= 3:
 *   interior, 0 < k < n-1: d[k] = 0 if sign(m[k-1]) != sign(m[k]) or either is 0; else with w1 = 2 h[k] + h[k-1] and
 *     w2 = h[k] + 2 h[k-1]:  d[k] = (w1 + w2) / (w1 / m[k-1] + w2 / m[k]).
 *   ends, with (h0, m0) the end segment and (h1, m1) its neighbour -- (h[0], m[0], h[1], m[1]) for d[0], (h[n-2], m[n-2], h[n-3],
 *     m[n-3]) for d[n-1]:  d = ((2 h0 + h1) m0 - h0 m1) / (h0 + h1);  0 if sign(d) != sign(m0);  else 3 m0 if sign(m0) != sign(m1)
 *     and |d| > 3 |m0|.
 *   frame t <= key[0]: y[0].   frame t >= key[n-1]: y[n-1].   Otherwise with k the largest index whose key[k] <= t, h = h[k],
 *     s = (t - key[k]) / h and u = 1 - s:
 *     h00 = ((1 + 2 s) u) u,  h10 = (s u) u,  h01 = (s s) (3 - 2 s),  h11 = (s s) (s - 1),
 *     v = (h00 y[k] + h10 (h d[k])) + (h01 y[k+1] + h11 (h d[k+1])).
 *   At a key s = 0 and v is the point itself; between two equal waypoints both slopes are 0 and v rounds to the point.
 *
 * ---- outputs ---------------------------------------------------------------------------------------------------------------------------
 * traj [b][dn][frames][2] float32: v, in metres.
 * x0 [b][frames dn][3] float32, row = frame dn + dancer (the layout of io.x0_from_trajectory and of tcdiff_nav_handoff): channel c of
 *   0, 1 is n = v scale[c] + min_[c] of the float64 v, -1 if n < -1, 1 if n > 1 (io.Normalizer clips, tcdiff_pose_export clamps),
 *   rounded once; with scale and min_ NULL it is traj's float.  Channel 2 is 0.  scale, min_: two HOST floats each, the normaliser's
 *   numbers of the two columns; they travel as kernel arguments.
 * Per (clip, dancer): status int32;  clamped int32: the frames with a channel that the clamp changed ("this formation lies outside
 *   anything the model was trained on");  with step[t] = sqrt(dx dx + dy dy) of the float32 values stored in traj, dx = traj[t+1][0] -
 *   traj[t][0], for t = 0 .. frames-2, a step that is not finite left out:  speed_max float64 = the largest step[t] fps (m/s) and
 *   speed_peak int32 its t, over a total order: the larger value, then the lower frame; without a step NaN and -1;  too_fast int32:
 *   the t with step[t] fps > max_speed;  path_length float64: the sum of the steps in the lane order of tcdiff_smooth.h -- lane l of
 *   64 adds the steps of t = l, l + 64, ... in ascending t to 0.0; the 64 lane sums are added in ascending lane order to 0.0.
 * Per (clip, pair i < j), in the order (0,1), (0,2), ..., (1,2), ... of group_metrics.pairs: over the frames in which the four floats
 *   of traj are finite, dist[t] = sqrt(dx dx + dy dy) of dancer j's minus dancer i's:  dist_min float64 and dist_min_frame int32: the
 *   smaller value, then the lower frame; with no frame left NaN and -1;  too_close int32: the frames with dist[t] < min_distance.
 *   With dn = 1 there is no pair: the three pointers may be NULL and the second launch is skipped.
 *
 * ---- the launches (csrc/choreo.hip) ---------------------------------------------------------------------------------------------------
 * 1. one workgroup of 256 per (clip, dancer): thread k checks key k and its point; the keys as int32 and the points and slopes as
 *    float64 go to LDS (9 KiB at 256 keys); then a thread per frame, TC_CHOREO_TILE frames at a time, finds its segment by binary
 *    search in LDS, evaluates, stores traj and x0; the tile's stored floats stay in LDS for the steps, which the first wave adds.
 * 2. one workgroup of 256 per (clip, pair) over traj.
 *
 * The checks, in this order.  TC_ERR_ARG: a NULL pointer (counts may be NULL); b, dn, K or frames < 1; K > TC_CHOREO_MAX_KEYS; fps
 * outside (0, 1e6]; min_distance or max_speed negative or NaN; one of scale and min_ NULL and the other not.  TC_ERR_UNSUPPORTED:
 * more than 2^31 - 1 (clip, dancer, frame) triples or (clip, pair) pairs.  TC_ERR_ARG: dn > 1 and a NULL pair output.  TC_ERR_ALIGN:
 * a float64 output not aligned to 8 bytes, an int32 output not to 4.
 *
 * ==== 2. tcc_trajectory_error (one launch) =============================================================================================
 * joints: float32, read in place; component k of the root (joint 0) of (clip c, dancer d, frame t) is at
 * joints + c strides[0] + d strides[1] + t strides[2] + k (element strides, each >= 0).  traj [b][dn][T][2] float32, contiguous, in
 * metres.  up in 0 .. 2; a0 < a1 are the two components that are not `up`.  T >= 1.
 *   e[t] = sqrt(dx dx + dy dy),  dx = root[t][a0] - traj[t][0],  dy = root[t][a1] - traj[t][1].
 * A frame whose e is not finite -- that is, one with a non-finite input among the four -- is counted out.
 *   traj_frames = the frames counted;  traj_err_mean = the sum of e in the lane order above / traj_frames;  traj_err_max and
 *   traj_err_peak: the larger value, then the lower frame;  traj_err_final: e of the last counted frame.  With no frame counted: NaN,
 *   NaN, NaN and -1.
 * One workgroup of 256 per (clip, dancer).
 * The checks, in this order.  TC_ERR_ARG: a NULL pointer; b, dn or T < 1; up outside 0 .. 2.  TC_ERR_UNSUPPORTED: more than 2^31 - 1
 * (clip, dancer, frame) triples.  TC_ERR_ARG: a negative stride.  TC_ERR_ALIGN: a float64 output not aligned to 8 bytes, an int32
 * output not to 4. */
#ifndef TCDIFF_CHOREO_H
#define TCDIFF_CHOREO_H

#include "tcdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TC_CHOREO_LAUNCHES 2
#define TC_CHOREO_TILE 256
#define TC_CHOREO_MAX_KEYS 256

/* traj [b][dn][frames][2], x0 [b][frames dn][3] float32; status, clamped, speed_peak, too_fast [b dn] int32; speed_max, path_length
 * [b dn] float64; dist_min [b pairs] float64, dist_min_frame, too_close [b pairs] int32 */
int tcc_plan(const float* points, const int* keys, int keys_per_dancer, const int* counts, int b, int dn, int K, int frames, double fps,
             const float* scale, const float* min_, double min_distance, double max_speed, float* traj, float* x0, int* status,
             int* clamped, double* speed_max, int* speed_peak, int* too_fast, double* path_length, double* dist_min,
             int* dist_min_frame, int* too_close, hipStream_t stream);

/* err_mean, err_max, err_final [b dn] float64; err_peak, counted [b dn] int32 */
int tcc_trajectory_error(const float* joints, const long* joint_strides, const float* traj, int b, int dn, int T, int up, double* err_mean,
                         double* err_max, double* err_final, int* err_peak, int* counted, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TCDIFF_CHOREO_H */
