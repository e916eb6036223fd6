/* tcdiff_hip_ext.h -- the second header of libtcdiff_gfx950.so's C ABI: launchers added after tcdiff_hip.h was pinned.  The
 * conventions of tcdiff_hip.h hold: every function returns 0 or a negative TC_ERR_* code, nothing is allocated, nothing
 * synchronises the host, pointers are caller-owned DEVICE pointers unless marked HOST, work is enqueued on `stream`.
 * Bound by tcdiff_amd/_lib.py next to the first header (ABI of the first, EXT of this one).
 */
#ifndef TCDIFF_HIP_EXT_H
#define TCDIFF_HIP_EXT_H

#include "tcdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- geometric features (csrc/geometric.hip, csrc/geo_math.h) -------------------------------------------------------------------
 * The relational (Mueller-style boolean) features on which Bailando and FACT report FID_g and Div_g, as a table-driven
 * evaluator: R rows of a predicate on a few points of a frame, each feature the fraction of frames at which its predicate holds.
 * The kinds and the default table below are restated from memory of the AIST++ API (aist_plusplus/features/{manual,utils}.py) and
 * of Bailando's copy; neither is a dependency, and parity with the packages' own output is NOT pinned.
 *
 * tcdiff_geometric_features, one launch.  joints (b, dn, T, 24, 3) fp32 DEVICE read in place through joint_strides (HOST long[3],
 * element strides of b, dn, T; the trailing 24 x 3 run is contiguous) exactly as tcdiff_kinetic_features reads it.  table [R][5]
 * int DEVICE: (kind, a, b, c, p) per row; range [R][2] double DEVICE: (lo, hi) per row; 1 <= R <= TC_SET_MAX_D.
 * feats [b][dn][R] double DEVICE: feats[.][.][r] = (the number of frames t = 1 .. T - 1 at which row r holds) / (T - 1), the
 * count an integer converted to double, so any order of counting gives the same bits.  T < 2: all R values NaN.
 *
 * Points.  Frame t has TC_GEO_POINTS = 28 points P_t[0 .. 27], float64:
 *   0 .. 23  the frame's joints: root, lhip, rhip, belly, lknee, rknee, spine, lankle, rankle, chest, ltoes, rtoes, neck,
 *            linshoulder, rinshoulder, head, lshoulder, rshoulder, lelbow, relbow, lwrist, rwrist, lhand, rhand
 *   24       zero
 *   25       up: 1 in component `up`, 0 in the two others;   26  -up: its negative
 *   27       floor: 0 in the two horizontal components, and in component `up` the minimum of that frame's 24 joints' `up`
 *            component (NaN if one of them is NaN)
 * a, b, c, p below are P_t[a] .. P_t[p]; a', p' the same points of frame t - 1; tau = time_per_frame.
 *   x - y componentwise;  dot(x, y) = (x0 y0 + x1 y1) + x2 y2;  |x| = sqrt(dot(x, x));
 *   x cross y = (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0)
 *
 * Kinds.
 *   TC_GEO_PLANE   n = (c - a) cross (b - a);  v = dot(n, p - a) / |n|                          holds when v > lo
 *   TC_GEO_NPLANE  n = b - a;                  v = dot(n, p - c) / |n|                          holds when v > lo
 *   TC_GEO_MOVE    w = (p - a) - (p' - a');  n = b - a;  v = dot(w, n) / |n| / tau  (c is not read)   holds when v > lo
 *   TC_GEO_NMOVE   w as above;  n = (c - a) cross (b - a);  v = dot(w, n) / |n| / tau                 holds when v > lo
 *   TC_GEO_ANGLE   u = b - a, w = p - c;  v = acos(min(max(dot(u, w) / (|u| |w|), -1), 1)) 180 / pi   holds when lo < v < hi
 *   TC_GEO_FAST    v = |p - p'| / tau  (only p is read)                                               holds when v > lo
 * A predicate whose v is not finite does not hold: a zero-length normal, a NaN joint.  Arithmetic is float64 on the float32
 * inputs, without contraction.  An implementation may decide TC_GEO_ANGLE on cosines instead of calling acos; away from ties
 * the result is the same.  A row whose kind is outside 0 .. 5 or one of whose four point indices is outside 0 .. 27 counts
 * nothing (its feature is 0) and nothing is read through it; callers refuse such tables before they upload them.
 *
 * The default table (tcdiff_amd/set_metrics.py GEOMETRIC_TABLE; data there, not code here): Bailando's 32 features.  Thresholds
 * are multiples of three lengths of the SMPL rest pose the AIST++ API hard-codes, computed on the host in float64:
 *   hl = |lshoulder - lelbow| = 0.25683810921...,  lshoulder (0.199113488, 0.236807942, -0.0180702247),
 *                                                  lelbow (0.454445392, 0.221158922, -0.0410167128)
 *   sw = |lshoulder - rshoulder| = 0.39084835854..., rshoulder (-0.191692337, 0.236928746, -0.0123055102)
 *   hw = |lhip - rhip| = 0.11924706586...,         lhip (0.0564076714, -0.323069185, 0.0109197125),
 *                                                  rhip (-0.0624834076, -0.331302464, 0.0150412619)
 *    #  kind    a          b          c          p        lo (, hi)
 *    0  NMOVE   neck       rhip       lhip       rwrist   1.8 hl
 *    1  NMOVE   neck       lhip       rhip       lwrist   1.8 hl
 *    2  NPLANE  chest      neck       neck       rwrist   0.2 hl
 *    3  NPLANE  chest      neck       neck       lwrist   0.2 hl
 *    4  MOVE    belly      chest      (rwrist)   chest    1.8 hl
 *    5  MOVE    belly      chest      (lwrist)   chest    1.8 hl
 *    6  ANGLE   relbow     rshoulder  relbow     rwrist   0, 110
 *    7  ANGLE   lelbow     lshoulder  lelbow     lwrist   0, 110
 *    8  NPLANE  lshoulder  rshoulder  lwrist     rwrist   2.5 sw
 *    9  MOVE    lwrist     rwrist     (lwrist)   rwrist   1.4 hl
 *   10  MOVE    rwrist     root       (root)     lwrist   1.4 hl
 *   11  MOVE    lwrist     root       (root)     rwrist   1.4 hl
 *   12  FAST                                     rwrist   2.5 hl
 *   13  FAST                                     lwrist   2.5 hl
 *   14  PLANE   root       lhip       ltoes      rankle   0.38 hl
 *   15  PLANE   root       rhip       rtoes      lankle   0.38 hl
 *   16  NPLANE  zero       up         floor      rankle   1.2 hl
 *   17  NPLANE  zero       up         floor      lankle   1.2 hl
 *   18  NPLANE  lhip       rhip       lankle     rankle   2.1 hw
 *   19  ANGLE   rknee      rhip       rknee      rankle   0, 110
 *   20  ANGLE   lknee      lhip       lknee      lankle   0, 110
 *   21  FAST                                     rankle   2.5 hl
 *   22  FAST                                     lankle   2.5 hl
 *   23  ANGLE   neck       root       rshoulder  relbow   25, 180
 *   24  ANGLE   neck       root       lshoulder  lelbow   25, 180
 *   25  ANGLE   neck       root       rhip       rknee    50, 180
 *   26  ANGLE   neck       root       lhip       lknee    50, 180
 *   27  PLANE   rankle     neck       lankle     root     0.5 hl
 *   28  ANGLE   neck       root       zero       up       70, 110
 *   29  NPLANE  zero       -up        floor      rwrist   -1.2 hl
 *   30  NPLANE  zero       -up        floor      lwrist   -1.2 hl
 *   31  FAST                                     root     2.3 hl
 * Two quirks of the package are kept on purpose, because published numbers carry them.  Rows 4, 5 and 9 - 11: the package's
 * f_move(j1, j2, j3, j4) hands j3, not j4, to the velocity test, so the point that moves is the third name and the fourth (in
 * brackets: the c column, which TC_GEO_MOVE does not read) is ignored.  And the package's time per frame is a hard-coded 1 / 120
 * whatever the clip's frame rate; that is the Python default of time_per_frame.  The blank entries of the FAST rows are not read;
 * the default table stores the row's p there.
 *
 * TC_ERR_ARG for a NULL pointer, b, dn, T or R < 1, up outside 0..2, a time_per_frame that is not positive and finite;
 * TC_ERR_UNSUPPORTED for R > TC_SET_MAX_D or b * dn above 2^31 - 1.  The checks precede any GPU call. */
#define TC_GEO_PLANE 0
#define TC_GEO_NPLANE 1
#define TC_GEO_MOVE 2
#define TC_GEO_NMOVE 3
#define TC_GEO_ANGLE 4
#define TC_GEO_FAST 5
#define TC_GEO_POINTS 28
int tcdiff_geometric_features(const float* joints, const long* joint_strides, int b, int dn, int T, int up, const int* table,
                              const double* range, int R, double time_per_frame, double* feats, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TCDIFF_HIP_EXT_H */
