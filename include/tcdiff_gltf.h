/* tcdiff_gltf.h -- the third header of libtcdiff_gfx950.so's C ABI: the key-frame data of an animated glTF 2.0 file.  The
 * conventions of tcdiff_hip.h hold: every function returns 0 or a negative TC_ERR_* code, nothing is allocated, nothing
 * synchronises the host, pointers are caller-owned DEVICE pointers, work is enqueued on `stream`.
 *
 * Why the function is tcx_*, not tcdiff_*: the set of tcdiff_* symbols the library exports is frozen.  tcdiff_hip.h is pinned at
 * its 79 functions and tcdiff_hip_ext.h at its one, and the binding's EXPORTS list, which the tests hold equal to every dynamic
 * tcdiff_* symbol of the built library, is pinned at those 80.  Launchers added from here on take the prefix tcx_ and a header
 * of their own; tcdiff_amd/_lib.py binds this one as GLTF next to ABI and EXT and adds it to neither of them nor to EXPORTS.
 */
#ifndef TCDIFF_GLTF_H
#define TCDIFF_GLTF_H

#include "tcdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- glTF animation block (csrc/gltf.hip, csrc/gltf_math.h) ---------------------------------------------------------------------
 * What the reference's Blender_Visulization/src/FbxReadWriter.py addAnimation computes for an FBX file, as the one binary block
 * a .glb file's animation accessors point into: per-joint local rotations as quaternions, the root's rotation and translation
 * turned from the data's Z-up to glTF's Y-up, key frames at `fps`.  tcdiff_amd/gltf.py wraps the block into the container.
 *
 * Inputs, as tcdiff_pose_export writes them (frame-major, dancer-minor; clips = 1 in long mode) and as the fk_out pickles hold
 * them:  smpl_poses [clips][T][dn][24][3] fp32 axis-angle;  smpl_trans [clips][T][dn][3] fp32.
 *
 * Output.  out [clips][F] fp32, F = TC_GLTF_FLOATS(T, dn) = T (1 + 99 dn); a clip's F floats are
 *   times [T]                      times[t] = (float)((double)t / fps)
 *   then per dancer d = 0 .. dn - 1 (99 T floats each):
 *     trans [T][3]                 (x, z, -y) of smpl_trans[.][t][d]: the turn by -90 degrees about x; copies and one negation
 *     rot   [24][T][4]             joint-major, then frame: the quaternion (x, y, z, w), glTF's component order
 *
 * Quaternion of the rotation vector r = (r0, r1, r2).  float64 arithmetic on the float32 inputs, without contraction, each
 * component rounded to float32 once, at the store:
 *   t2 = (r0 r0 + r1 r1) + r2 r2;   theta = sqrt(t2);   a2 = theta theta
 *   k = (0.5 - a2 / 48) + a2 a2 / 3840     if theta < 1e-3,   else  sin(theta / 2) / theta
 *   q = (k r0, k r1, k r2, cos(theta / 2))
 * (scipy's Rotation.from_rotvec).  Joint 0 only: q <- f (x) q, the Hamilton product with f = (fx, 0, 0, fw) on the left,
 * fx = -sqrt(1/2) = -0.70710678118654757, fw = 0.70710678118654757 (FbxReadWriter.py:67,80 with the constant at full precision):
 *   x' = fw x + fx w;   y' = fw y - fx z;   z' = fw z + fx y;   w' = fw w - fx x
 * The bone offsets are not turned: SMPL's rest pose is Y-up already, only the root carries the data's Z-up.
 *
 * Sign continuity.  Per channel (clip, dancer, joint), q_t the float64 quaternion above:
 *   s_0 = -1 if w_0 < 0, else +1
 *   s_t = -s_(t-1) if ((x_t x_(t-1) + y_t y_(t-1)) + z_t z_(t-1)) + w_t w_(t-1) < 0, else s_(t-1)
 * and what is stored is (float)(s_t q_t), so that an importer which interpolates components never turns a joint the long way
 * round.  A zero or NaN dot product (and a NaN w_0) does not flip.  s_t is the parity of the number of flips up to t: the
 * kernel takes it from a wave's ballot, and the same input gives the same bits.
 *
 * TC_ERR_ARG for a NULL pointer, clips, T or dn < 1, an fps that is not positive and finite; TC_ERR_UNSUPPORTED when clips * F
 * (which is above the element count of either input) is above 2^31 - 1.  The checks precede any GPU call. */
#define TC_GLTF_FLOATS(T, dn) ((long)(T) * (1L + 99L * (long)(dn)))
int tcx_gltf_animation(const float* smpl_poses, const float* smpl_trans, int clips, int T, int dn, double fps, float* out,
                       hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TCDIFF_GLTF_H */
