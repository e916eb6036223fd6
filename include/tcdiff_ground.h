/* tcdiff_ground.h -- the tenth header of libtcdiff_gfx950.so's C ABI: PUTTING THE DANCERS ON THE FLOOR.  A floor measure and a
 * post-process on what tcdiff_pose_export (or tcp_keep_apart) leaves on the device: each dancer's root is shifted VERTICALLY so that
 * its planted feet stand on the floor and no part of its body sinks below it, the shift eased in and out in time; rotations and the
 * two floor components are untouched, and the launch reports what it did and what it could not do.  The conventions of tcdiff_hip.h
 * hold: every function returns 0 or a negative TC_ERR_* code, nothing is allocated, nothing synchronises the host, pointers are
 * caller-owned DEVICE pointers (`joint_strides`, `contact_strides`, `parents`, `radii` and `bytes` excepted: HOST), work is enqueued
 * on `stream`, the checks precede any GPU call.
 *
 * Why the functions are tcf_*: the sets of tcdiff_*, tcx_*, tcs_*, tcr_*, tcj_*, tck_*, tcg_* and tcp_* symbols the library exports
 * are frozen (the tests hold each equal to the built library's dynamic symbols).  This header takes a prefix of its own;
 * tcdiff_amd/_lib.py binds it as GROUND next to ABI, EXT, GLTF, SKIN, SHADE, MJPEG, FOOTLOCK, GROUP and APART and adds it to none of
 * them nor to EXPORTS.
 *
 * The reference has no counterpart (it renders the raw poses); the construction is the project's own, in the spirit of the
 * "penetrate" and "float" scores of the physics-plausibility literature, parity with any other tool is unpinned, and what follows is
 * the definition.  tests/ground_ref.py is its numpy restatement.  tolerance, blend, max_lift and the default radii are choices, not
 * measurements.
 * Not built: mesh-level soles from skin's vertices; sloped or uneven floors; a floor per dancer; bending knees to absorb a correction;
 * correcting inside the sampler; drawing the grid at the estimated floor.
 *
 * ---- input ----------------------------------------------------------------------------------------------------------------------
 * joints: float32, read in place: joint j, component k of (clip c, dancer d, frame t) is at joints + c strides[0] + d strides[1] +
 * t strides[2] + 3 j + k (element strides, each >= 0).  pos: float32 [b][T dn][3], row = frame dn + dancer, contiguous.  contacts:
 * NULL, or float32 read in place, channel k of (c, d, t) at contacts + c strides[0] + d strides[1] + t strides[2] + k strides[3]; the
 * channels are the joints 7, 8, 10, 11 in this order, as in tcdiff_footlock.h.  parents [24] and radii [24] as in tcdiff_group.h:
 * bone i = 1 .. 23 joins parents[i] and i and has the radius radii[i].  floor_in: NULL (estimate the floor) or [b] float64.
 * All arithmetic is float64 on the float32 inputs, every product, quotient and sum rounded on its own (no contraction).  "z" is the
 * component `up`; a minimum of numbers is exact, so its order is free.
 *
 * ---- the definition, per clip c, dancer d, frame t ------------------------------------------------------------------------------
 * 1. Good frames.  A frame whose 72 joint words are all finite is good; any other is bad.  A bad frame's output words are its input's,
 *    its shift is 0, it takes part in no floor estimate and no metric, and for everything else it is an unplanted frame, e = 0.
 * 2. Body low.  L(t) = min over i = 1 .. 23 of (min(z[parents[i]], z[i]) - radii[i]).
 * 3. Labels.  Left foot planted: contacts[0] > contact_threshold or contacts[2] > contact_threshold (float32 compares); right foot:
 *    channels 1 and 3.  Without contacts, joint j is still at t if t = T - 1, or if sqrt((dx dx + dy dy) + dz dz) < still with
 *    (dx, dy, dz) = P_j[t + 1] - P_j[t] (the dataset's rule, as tcdiff_footlock.h applies it; a bad frame t + 1 gives a NaN: not
 *    still); the left foot is planted if joint 7 or joint 10 is still, the right if 8 or 11 is.  Only a good frame has a planted foot.
 *    Foot lows: lo_l = min(z[7], z[10]) - radii[10], lo_r = min(z[8], z[11]) - radii[11].  A frame is planted if a foot is;
 *    Lf(t) = the minimum of the planted feet's lows.  The labels are decided once, on the input: "after" uses the same labels.
 * 4. Floor F of a clip.  floor_in[c] if given.  Otherwise numpy's median of the multiset of planted foot lows (one value per planted
 *    foot, over every dancer and frame of the clip): the middle value, or (lo + hi) / 2 of the two middle ones; if the clip has no
 *    planted foot, the same median of L over its good frames; NaN if it has no good frame either.  The selection is exact: the
 *    order-preserving 64-bit keys of the values, a digit at a time.  If F is not finite, no frame of the clip moves.
 * 5. Base shift B.  A run is a maximal sequence of planted frames.  In a run, B = (sum over its frames, in ascending t from 0, of
 *    a(s) = F - Lf(s)) / (its length).  An unplanted frame t with a run ending at i < t before it and one starting at j > t after it:
 *    if j - i - 1 <= 2 blend, B(t) = B(i) + (B(j) - B(i)) ((t - i) / (j - i)); otherwise, and where one of the two is absent,
 *    B(t) = B(i) w(t - i) if the earlier run exists and t - i <= blend, else B(j) w(j - t) if the later one exists and
 *    j - t <= blend, else 0.  w(k) = 1 - k / (blend + 1), the quotient and the difference in float64 (w(0) = 1 exactly).
 * 6. Lift.  e(t) = max((F - L(t)) - B(t), 0) on a good frame, 0 on a bad one.  U(t) = max over |s - t| <= blend, 0 <= s < T, of
 *    e(s) w(|s - t|).  D(t) = B(t) + U(t), clamped to [-max_lift, max_lift]; a frame clamped is CAPPED.  D = 0 on a bad frame and on
 *    every frame of a clip whose F is not finite.  So L(t) + D(t) >= F on every uncapped good frame, up to rounding; a jump further
 *    than blend frames from every run and from every frame with an excess is left alone.
 * 7. Output.  Where D(t) == 0 the output words of (c, d, t) -- its row of pos_out and its 24 joints -- are the input's words, copied
 *    without arithmetic (a -0.0 stays -0.0, a NaN keeps its payload).  Elsewhere the `up` component x of pos and of the 24 joints is
 *    float32(float64(x) + D(t)); the other two components are the input's words.
 * 8. Metrics, per (clip, dancer), with F as above and the labels of step 3; sums in ascending t from 0:
 *    counts[0] planted frames; counts[1] penetration frames: good frames with L < F - tolerance; counts[2] float frames: planted
 *    frames with Lf > F + tolerance.  values[0] penetration max: the maximum over good frames of max(F - L, 0), 0 if there is none;
 *    values[1] penetration mean: the sum of max(F - L, 0) over good frames / their count (NaN for none); values[2] float mean: the
 *    sum of max(Lf - F, 0) over planted frames / their count (NaN for none).  Where F is not finite counts[1], counts[2] are 0 and
 *    the three values NaN.  "before" is evaluated on the input, "after" on the float32 outputs with the labels of the input.
 *    capped: the frames capped; max_shift = max over t of |D(t)|; max_step = max over t >= 1 of |D(t) - D(t - 1)|, 0 for T = 1.
 *
 * ---- the launchers (csrc/ground.hip) -----------------------------------------------------------------------------------------------
 * TC_GROUND_LAUNCHES launches whatever b is (one less with floor_in), TC_GROUND_METRICS_LAUNCHES for tcf_ground_metrics (likewise);
 * no atomics, every sum in one order, every minimum and maximum exact: the same input gives the same bits.
 *   frames: one thread per (clip, dancer, frame): good, L, the foot lows and the labels into the workspace.
 *   median: one workgroup per clip (skipped with floor_in): the keys of the candidates, the first TC_GROUND_MEDIAN_KEYS of them
 *           staged in LDS and the rest read again from the workspace, TC_GROUND_DIGIT_BITS bits a pass, the digit counts reduced by
 *           wave shuffles; writes floor.
 *   walk:   one wave per (clip, dancer), frames in chunks of 64: the runs (a lane at a run's first frame sums it in ascending t),
 *           the nearest planted frame before and after each frame from wave ballots, then B, e, U and D.
 *   apply:  one thread per (clip, dancer, frame): the copy rule above, then L and the foot lows of the float32 output.
 *   stats:  one wave per (clip, dancer) and evaluation (before, after): counts and maxima over the lanes, each sum by one lane in
 *           ascending t; the wave of (clip, dancer 0, before) copies floor_in to floor.
 * workspace: TC_GROUND_WS_PER_FRAME bytes per (clip, dancer, frame) -- nine float64 planes (L, the two foot lows before and after,
 *   B, e, D) and a flag byte -- rounded up to a multiple of 8, aligned to 8; tcf_ground_metrics needs the same.
 *
 * The checks, in this order.  TC_ERR_ARG: a NULL pointer (contacts, contact_strides, floor_in and shift may be NULL; contact_strides
 * must not be if contacts is not); b, dn or T < 1; up outside 0..2; blend negative; a NaN contact_threshold; still, tolerance or
 * max_lift negative or not finite.  TC_ERR_UNSUPPORTED: dn > TC_GROUND_MAX_DANCERS; blend > TC_GROUND_MAX_BLEND; more than 2^31 - 1
 * (clip, dancer, frame) triples.  TC_ERR_ARG: a negative stride; a parent of joint 1 .. 23 that is negative or does not precede its
 * child; a radius of bone 1 .. 23 that is negative or not finite; workspace_bytes below tcf_ground_workspace's.  TC_ERR_ALIGN:
 * workspace, floor_in or shift not aligned to 8 bytes.
 * tcf_ground_workspace: TC_ERR_ARG for a NULL `bytes`, the same shape checks, TC_ERR_UNSUPPORTED likewise. */
#ifndef TCDIFF_GROUND_H
#define TCDIFF_GROUND_H

#include "tcdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TC_GROUND_LAUNCHES 5
#define TC_GROUND_METRICS_LAUNCHES 3
#define TC_GROUND_MAX_DANCERS 32
#define TC_GROUND_MAX_BLEND 1024
#define TC_GROUND_WS_PER_FRAME 73
#define TC_GROUND_MEDIAN_KEYS 4096
#define TC_GROUND_DIGIT_BITS 4
#define TC_GROUND_LEFT 1
#define TC_GROUND_RIGHT 2
#define TC_GROUND_GOOD 4
#define TC_GROUND_CAPPED 8

/* bytes[0] (a HOST long) = the workspace tcf_ground and tcf_ground_metrics need for b clips of dn dancers and T frames */
int tcf_ground_workspace(int b, int dn, int T, long* bytes);

/* floor [b] float64: F as used; counts [3][b dn] int64 (long), values [3][b dn] float64: the metrics of step 8 on joints. */
int tcf_ground_metrics(const float* joints, const long* joint_strides, const float* contacts, const long* contact_strides, int b,
                       int dn, int T, int up, const int* parents, const double* radii, const double* floor_in,
                       float contact_threshold, double still, double tolerance, void* workspace, long workspace_bytes, double* floor,
                       long* counts, double* values, hipStream_t stream);

/* pos_out [b][T dn][3] and joints_out [b][dn][T][24][3] float32; shift [b][dn][T] float64, D, or NULL; floor [b] float64;
 * counts_before / counts_after [3][b dn] int64, values_before / values_after [3][b dn] float64; capped [b dn] int64;
 * max_shift, max_step [b dn] float64. */
int tcf_ground(const float* pos, const float* joints, const long* joint_strides, const float* contacts, const long* contact_strides,
               int b, int dn, int T, int up, const int* parents, const double* radii, const double* floor_in, float contact_threshold,
               double still, double tolerance, int blend, double max_lift, void* workspace, long workspace_bytes, float* pos_out,
               float* joints_out, double* shift, double* floor, long* counts_before, double* values_before, long* counts_after,
               double* values_after, long* capped, double* max_shift, double* max_step, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TCDIFF_GROUND_H */
