/* tcdiff_skin.h -- the fourth header of libtcdiff_gfx950.so's C ABI: the vertices of a user-supplied SMPL body, skinned on the
 * device.  The conventions of tcdiff_hip.h hold: every function returns 0 or a negative TC_ERR_* code, nothing is allocated,
 * nothing synchronises the host, pointers are caller-owned DEVICE pointers (`parents` excepted), work is enqueued on `stream`.
 *
 * Why the function is tcs_*: the set of tcdiff_* symbols the library exports is frozen at 80 and the set of tcx_* symbols at the
 * one of tcdiff_gltf.h (the tests hold both equal to the built library's dynamic symbols).  This header takes a prefix of its
 * own; tcdiff_amd/_lib.py binds it as SKIN next to ABI, EXT and GLTF and adds it to none of them nor to EXPORTS.
 *
 * The model file is the user's: nothing of it is shipped.  Parity with smplx and with the official model files is unpinned
 * (neither is a dependency); what follows restates Loper et al. 2015 as smplx evaluates it, and is what the tests hold the
 * kernels to.
 */
#ifndef TCDIFF_SKIN_H
#define TCDIFF_SKIN_H

#include "tcdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- linear blend skinning of an SMPL body (csrc/skin.hip, csrc/skin_math.h) -------------------------------------------------------
 * The model, prepared once on the host in float64 (tcdiff_amd/body.py) and rounded to float32 once when uploaded:
 *   v_shaped [V][3]     v_template + shapedirs . betas
 *   blend    [207][3V]  the pose-corrective blend shapes, blend[k][3v + c] = posedirs[v][c][k]
 *   joints   [24][3]    J = J_regressor . v_shaped (float64), the rest joints
 *   offsets  [24][3]    J[j] - J[parent[j]], zero for the root
 *   parents  [24]       a HOST array: the root's entry is any value outside 0..23, every other joint's parent comes before it
 *   weights  [V][K], weight_joints [V][K] (int)   per vertex its K skinning weights and their joints in ascending joint order,
 *                       padded with weight 0 on joint 0; 1 <= K <= 8
 * A pose is one (clip, frame, dancer) as tcdiff_pose_export numbers them: smpl_poses [P][24][3] fp32 axis-angle, smpl_trans
 * [P][3] fp32.
 *
 * Launch 1, one thread per pose.  float64 arithmetic on the float32 inputs, without contraction, every product and sum in the
 * order written, each result rounded to float32 once, at the store.
 *   Rotation of r = (r0, r1, r2):
 *     q = (r0 r0 + r1 r1) + r2 r2;   theta = sqrt(q);   t2 = theta theta
 *     a = sin(theta) / theta,  b = (1 - cos(theta)) / t2                            if theta >= 1e-3 (or NaN), else the series
 *     a = (1 - t2 / 6) + t2 t2 / 120,  b = (0.5 - t2 / 24) + t2 t2 / 720
 *     R = [ 1 - b (r1 r1 + r2 r2)    b (r0 r1) - a r2         b (r0 r2) + a r1      ]
 *         [ b (r0 r1) + a r2         1 - b (r0 r0 + r2 r2)    b (r1 r2) - a r0      ]
 *         [ b (r0 r2) - a r1         b (r1 r2) + a r0         1 - b (r0 r0 + r1 r1) ]
 *   feat [P][TC_SKIN_FEAT]:  feat[9 (j - 1) + 3 a + b] = R_j[a][b] - (a == b), j = 1 .. 23;  feat[207] = 0 (an even length)
 *   G_root = [R_root | J_root];   G_j = G_parent . [R_j | offsets[j]], joints in ascending order:
 *     G_j^R[a][b] = (Gp^R[a][0] R_j[0][b] + Gp^R[a][1] R_j[1][b]) + Gp^R[a][2] R_j[2][b]
 *     G_j^t[a]    = ((Gp^R[a][0] o[0] + Gp^R[a][1] o[1]) + Gp^R[a][2] o[2]) + Gp^t[a]
 *   A [P][24][12], row-major 3 x 4:  A_j = [G_j^R | G_j^t[a] - ((G_j^R[a][0] J_j[0] + G_j^R[a][1] J_j[1]) + G_j^R[a][2] J_j[2])]
 *   shift s = trans - J_root for origin = TC_SKIN_ORIGIN_PELVIS (the pelvis sits at smpl_trans, as in tcdiff_pose_export's
 *     joints and in the .glb's root node), s = trans for TC_SKIN_ORIGIN_SMPL (SMPL's own convention)
 *   joints_out [P][24][3] (optional, may be NULL):  joints_out[j] = G_j^t + s
 *
 * Launch 2, a workgroup per TC_SKIN_POSE_TILE poses x TC_SKIN_VERT_TILE vertices, float32, per pose and vertex v:
 *   d[c]   = sum over k = 0 .. 207 of feat[k] blend[k][3v + c], ONE fused-multiply-add chain in ascending k from a zero accumulator
 *            (blend's row 207 is taken as zero; v_mfma_f32_32x32x2_f32 evaluates exactly this chain);  d = 0 when pose_blend = 0
 *   vp[c]  = v_shaped[v][c] + d[c]
 *   T[e]   = sum over the K slots in ascending slot order of w_s A_(j_s)[e], one fmaf chain from zero, e = 0 .. 11
 *   out[a] = (fmaf(T[a][2], vp[2], fmaf(T[a][1], vp[1], fmaf(T[a][0], vp[0], 0))) + T[a][3]) + (float)s[a]
 *   out [P][V][3] fp32, in the data's frame (Z-up) like the export's joints.  A vertex's bits do not depend on the tile or the batch
 *   it is computed in.  Plain stores, no atomics; nothing outside out, feat, A and joints_out is written.
 *
 * The checks precede any GPU call, in this order.  TC_ERR_ARG: a NULL pointer (joints_out excepted); P, V or K < 1, K > 8; a
 * pose_blend or origin flag out of range; a parent index >= its child's, no root or more than one.  TC_ERR_ALIGN: feat or A not
 * aligned to 16 bytes.  TC_ERR_UNSUPPORTED: P V 3 or P 24 12 above 2^31 - 1.  The joint indices of weight_joints live on the
 * device and are validated by the caller (tcdiff_amd/body.py load_body_model). */
#define TC_SKIN_POSE_TILE 32
#define TC_SKIN_VERT_TILE 128
#define TC_SKIN_FEAT 208
#define TC_SKIN_ORIGIN_PELVIS 0
#define TC_SKIN_ORIGIN_SMPL 1
int tcs_skin_vertices(const float* smpl_poses, const float* smpl_trans, int P, const float* v_shaped, const float* blend,
                      const float* joints, const float* offsets, const int* parents, const float* weights,
                      const int* weight_joints, int V, int K, int pose_blend, int origin, float* feat, float* A,
                      float* joints_out, float* out, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TCDIFF_SKIN_H */
