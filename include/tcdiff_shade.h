/* tcdiff_shade.h -- the fifth header of libtcdiff_gfx950.so's C ABI: shaded, depth-tested frames of triangle meshes (the skinned
 * SMPL bodies of tcdiff_skin.h), drawn on the device.  The conventions of tcdiff_hip.h hold: every function returns 0 or a negative
 * TC_ERR_* code, nothing is allocated, nothing synchronises the host, pointers are caller-owned DEVICE pointers (`view` and `style`
 * excepted), work is enqueued on `stream`, the checks precede any GPU call.
 *
 * Why the functions are tcr_*: the sets of tcdiff_*, tcx_* and tcs_* symbols the library exports are frozen (the tests hold each
 * equal to the built library's dynamic symbols).  This header takes a prefix of its own; tcdiff_amd/_lib.py binds it as SHADE next
 * to ABI, EXT, GLTF and SKIN and adds it to none of them nor to EXPORTS.
 *
 * Parity with any other renderer is unpinned: what follows is the project's own definition of the picture, as tcdiff_draw_raster's
 * is, and is what the tests hold the kernels to (tests/shade_ref.py restates it in numpy float64).  Not built: anti-aliasing,
 * perspective, textures, shadows.
 */
#ifndef TCDIFF_SHADE_H
#define TCDIFF_SHADE_H

#include "tcdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- screen positions and vertex normals of posed meshes (csrc/shade.hip) ----------------------------------------------------------
 * One launch, one thread per (pose, vertex).  A pose is one (clip, frame, dancer), row = frame * dn + dancer, as tcdiff_pose_export
 * and tcs_skin_vertices number them.
 *   vertices  [P][V][3] fp32     faces [F][3] int32
 *   adj_start [V + 1], adj_faces [3F] int32: per vertex v the faces that name it, adj_faces[adj_start[v] .. adj_start[v + 1]), in
 *             ascending face index (a face that names v twice is listed twice); built once on the host
 *   view[12]  a HOST array, row-major 3 x 4 as tcdiff_draw_project takes it
 *   screen  [P][V][3] fp32 (may be NULL):  screen[r] = fmaf(view[r][2], Z, fmaf(view[r][1], Y, fmaf(view[r][0], X, view[r][3]))),
 *             float32, three roundings: within 4 * 2^-24 * (|m0 X| + |m1 Y| + |m2 Z| + |m3|) of the exact value
 *   normals [P][V][3] fp32 (may be NULL):  s = the sum over v's adjacent faces, in the order adj_faces lists them, from zero, of
 *             e1 x e2 = (e1y e2z - e1z e2y,  e1z e2x - e1x e2z,  e1x e2y - e1y e2x),  e1 = p1 - p0,  e2 = p2 - p0
 *             with p0, p1, p2 the face's vertices in the face's order (area weighted);  len = sqrt((sx sx + sy sy) + sz sz);
 *             normal = s / len, or (0, 0, 0) when len = 0.  float64 arithmetic on the fp32 positions, without contraction, every
 *             product, difference and sum in the order written, each component rounded to fp32 once, at the store.  No atomics:
 *             a normal's bits do not depend on the launch shape.  A face index outside 0 .. F - 1 in adj_faces, or a face with a
 *             vertex index outside 0 .. V - 1, adds nothing (and nothing is read through it).
 * TC_ERR_ARG: a NULL vertices, faces or view; normals wanted without adj_start / adj_faces; both outputs NULL; P, V or F < 1.
 * TC_ERR_UNSUPPORTED: P V 3 or 3 F above 2^31 - 1. */
int tcr_mesh_vertices(const float* vertices, const int* faces, const int* adj_start, const int* adj_faces, int P, int V, int F,
                      const float* view, float* screen, float* normals, hipStream_t stream);

/* ---- the shaded, depth-tested picture (csrc/shade.hip) -------------------------------------------------------------------------------
 * TC_SHADE_RASTER_LAUNCHES launches, whatever the sizes.  Launch 1, one thread per triangle of every frame, writes the triangle's
 * pixel box into scratch, and per chunk of TC_SHADE_CHUNK consecutive triangles of a frame the union of its boxes; launch 2, grid
 * (tiles, T, b), one workgroup of 256 threads per TC_SHADE_TILE x TC_SHADE_TILE tile of one frame, walks the chunks whose box
 * meets the tile in ascending triangle index, keeps the triangles whose box meets it in LDS, and decides and shades its pixels.
 * No atomics anywhere; the kept list never exceeds a chunk, whatever falls into a tile.
 *   screen, normals [b][T * dn][V][3] fp32 as tcr_mesh_vertices writes them;  faces [F][3] int32
 *   colors [n_colors][3] uint8: dancer d takes colour d % n_colors
 *   style  a HOST struct: the background, ambient in [0, 1], light = a unit vector (| |light|^2 - 1 | <= 1e-3) in WORLD axes,
 *          the axes `normals` are given in
 *   under  [b][T][H][W][3] uint8 or NULL: the picture below the bodies
 *   scratch, scratch_bytes: at least TC_SHADE_SCRATCH_PER_TRIANGLE * b * T * (dn * F + ceil(dn * F / TC_SHADE_CHUNK)) bytes (a box
 *          per triangle and one per chunk), aligned to 8
 *   frames [b][T][H][W][3] uint8
 *
 * Triangle g = d * F + f of a frame has the screen vertices a, b, c = screen[frame][d][faces[f][0 .. 2]].  At the centre
 * (px, py) = (x + 0.5, y + 0.5) of pixel (x, y), all in float64 on the fp32 inputs, without contraction, in the order written:
 *   E_0 = (b.x - a.x) (py - a.y) - (b.y - a.y) (px - a.x)        [edge a b]
 *   E_1 = (c.x - b.x) (py - b.y) - (c.y - b.y) (px - b.x)        [edge b c]
 *   E_2 = (a.x - c.x) (py - c.y) - (a.y - c.y) (px - c.x)        [edge c a]
 *   area = (E_0 + E_1) + E_2
 * The triangle covers the pixel when area != 0, all E_i >= 0 or all E_i <= 0 (two-sided: winding and the y-down screen do not
 * matter), and the centre lies in the triangle's bounding box, min(a.x, b.x, c.x) <= px <= max(a.x, b.x, c.x) and the same in y --
 * a condition every covered point meets in exact arithmetic, and the one the tiles cull by, exactly, so that a pixel's bits depend
 * on neither tile nor chunk nor batch.  A triangle with a screen coordinate that is not finite, or a vertex index outside
 * 0 .. V - 1, covers nothing.
 *   depth   z = ((E_1 a.z + E_2 b.z) + E_0 c.z) / area            (a vertex's weight is the edge function opposite to it)
 *   The visible triangle is the covering one of smallest z; ties go to the smallest g.  (The rule does not depend on the order in
 *   which triangles are met.)
 *   shading n = (E_1 n_a + E_2 n_b) + E_0 n_c per component, on the fp32 normals of the three vertices (not divided by area: k does
 *           not depend on n's length);  dot = (n.x l.x + n.y l.y) + n.z l.z;  len = sqrt((n.x n.x + n.y n.y) + n.z n.z);
 *           k = ambient + (1 - ambient) (|dot| / len), or k = ambient when len = 0 or k is not a number
 *           channel c of the pixel = floor(colors[d % n_colors][c] k + 0.5), at most 255
 *   A pixel that no triangle covers takes under's pixel, or the background.
 * One sample per pixel, no anti-aliasing.  Plain stores; nothing outside frames and scratch is written.  Same input, same bits.
 *
 * The checks, in this order.  TC_ERR_ARG: a NULL pointer (under excepted); b, T, dn, V, F, W, H or n_colors < 1; ambient outside
 * [0, 1], a light that is not finite or not a unit vector.  TC_ERR_UNSUPPORTED: b or T above 65535 (as tcdiff_draw_raster), W or H
 * above TC_SHADE_MAX_SIDE (a box's four values share eight bytes), or b T dn V 3, b T dn F or b T H W 3 above 2^31 - 1.
 * TC_ERR_ARG: scratch_bytes below the formula.  TC_ERR_ALIGN: scratch not aligned to 8 bytes.
 * The vertex indices of faces live on the device: a bad one draws nothing, and tcdiff_amd/body.py load_body_model refuses it. */
#define TC_SHADE_TILE 32
#define TC_SHADE_CHUNK 256
#define TC_SHADE_RASTER_LAUNCHES 2
#define TC_SHADE_SCRATCH_PER_TRIANGLE 8
#define TC_SHADE_MAX_SIDE 32767
typedef struct {
    unsigned char background[3];
    float ambient;
    float light[3];
} tcr_shade_style;
int tcr_mesh_raster(const float* screen, const float* normals, const int* faces, int b, int T, int dn, int V, int F, int W, int H,
                    const unsigned char* colors, int n_colors, const tcr_shade_style* style, const unsigned char* under, int* scratch,
                    long scratch_bytes, unsigned char* frames, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TCDIFF_SHADE_H */
