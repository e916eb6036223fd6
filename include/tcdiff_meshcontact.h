/* tcdiff_meshcontact.h -- the eleventh header of libtcdiff_gfx950.so's C ABI: MESH-LEVEL CONTACT between the dancers' skinned bodies.
 * A measure on the vertices tcs_skin leaves on the device: per clip and pair of dancers, in how many frames the surface of one body
 * passes through the other's, how many vertices are inside and how deep the deepest one is.  The conventions of tcdiff_hip.h hold:
 * every function returns 0 or a negative TC_ERR_* code, nothing is allocated, nothing synchronises the host, pointers are
 * caller-owned DEVICE pointers (`vertex_strides`, `faces_host` and `bytes` excepted: HOST), work is enqueued on `stream`, the checks
 * precede any GPU call.
 *
 * Why the functions are tcm_*: the sets of tcdiff_*, tcx_*, tcs_*, tcr_*, tcj_*, tck_*, tcg_*, tcp_* and tcf_* symbols the library
 * exports are frozen (the tests hold each equal to the built library's dynamic symbols).  This header takes a prefix of its own;
 * tcdiff_amd/_lib.py binds it as MESH next to ABI, EXT, GLTF, SKIN, SHADE, MJPEG, FOOTLOCK, GROUP, APART and GROUND and adds it to
 * none of them nor to EXPORTS.
 *
 * The reference has no counterpart (it renders the raw poses); the construction is the textbook one -- a signed ray count for
 * "inside", Ericson's closest point of a triangle for the depth -- restated, parity with any other tool is unpinned, and what follows
 * is the definition.  tests/meshcontact_ref.py is its numpy restatement.
 * Not built: edge-edge crossings between vertices (a limb thinner than the vertex spacing can pass unseen); contact of a dancer with
 * itself; the gap between surfaces that do not touch; using any of this inside keep_apart or ground; a penetration volume; a spatial
 * hierarchy.
 *
 * ---- input ----------------------------------------------------------------------------------------------------------------------
 * vertices: float32, read in place: component k of vertex v of (clip c, frame t, dancer d) is at vertices + c strides[0] +
 * (t dn + d) strides[1] + 3 v + k (element strides, each >= 0).  faces: int32 [F][3], vertex indices in 0 .. V - 1, one mesh for
 * every dancer; faces_host is the same array in HOST memory, read by the checks alone.  All arithmetic is float64 on the float32
 * inputs, every product, quotient, sum and difference rounded on its own (no contraction).  With `up` the vertical axis, a point's
 * x is its component (up == 0 ? 1 : 0), its y the component (up == 2 ? 1 : 2), its z the component `up`.
 *
 * ---- the definition, per clip c, frame t and ORDERED pair (a -> b) of dancers, a != b ----------------------------------------------
 * 1. Valid frames.  A pose is finite if its 3 V words are.  The frame of a pair is valid iff both poses are finite.
 * 2. Edges.  For a point p and the edge of the vertices with the indices i < j, u = vertex i and w = vertex j of body b (ALWAYS in
 *    ascending index, whatever the face's order; an edge with i == j is never crossed): the edge straddles p iff
 *    (u.y > p.y) != (w.y > p.y); it is CROSSED iff it straddles and p.x < xe, xe = u.x + ((p.y - u.y) / (w.y - u.y)) (w.x - u.x).
 *    Two faces that share an edge make the same decision about it, bit for bit.
 * 3. Covering.  A face (i0, i1, i2) with A, B, C = the vertices i0, i1, i2 COVERS p iff an odd number of its edges {i0, i1},
 *    {i1, i2}, {i2, i0} is crossed.
 * 4. Height and sign of a covering face.  D = (B.x - A.x) (C.y - A.y) - (B.y - A.y) (C.x - A.x);
 *    l1 = ((p.x - A.x) (C.y - A.y) - (p.y - A.y) (C.x - A.x)) / D;  l2 = ((B.x - A.x) (p.y - A.y) - (B.y - A.y) (p.x - A.x)) / D;
 *    z_hit = (A.z + l1 (B.z - A.z)) + l2 (C.z - A.z).  A covering face with D == 0 contributes nothing (the products of float32
 *    differences are exact in float64, so the sign of D is the true one and a face that truly covers has D != 0).
 * 5. Inside.  w(p) = the sum over the covering faces with z_hit > p.z of (D > 0 ? 1 : -1): a winding number, not a parity, so a place
 *    where b's own surface folds through itself does not turn into "outside".  The vertex is INSIDE b iff w(p) != 0.
 * 6. Depth of an inside vertex: the minimum over ALL F faces of the distance from p to the triangle, dist = sqrt((e.x e.x + e.y e.y)
 *    + e.z e.z), e = p - q, q the closest point of the triangle in Ericson's regions (x, y, z as above, whatever `up` is;
 *    a . b = (a.x b.x + a.y b.y) + a.z b.z; s m = (s m.x, s m.y, s m.z); the first region that applies):
 *      ab = B - A, ac = C - A, ap = p - A, d1 = ab . ap, d2 = ac . ap;               d1 <= 0 and d2 <= 0: q = A
 *      bp = p - B, d3 = ab . bp, d4 = ac . bp;                                       d3 >= 0 and d4 <= d3: q = B
 *      vc = d1 d4 - d3 d2;                            vc <= 0 and d1 >= 0 and d3 <= 0: q = A + (d1 / (d1 - d3)) ab
 *      cp = p - C, d5 = ab . cp, d6 = ac . cp;                                       d6 >= 0 and d5 <= d6: q = C
 *      vb = d5 d2 - d1 d6;                            vb <= 0 and d2 >= 0 and d6 <= 0: q = A + (d2 / (d2 - d6)) ac
 *      va = d3 d6 - d5 d4, g = d4 - d3, h = d5 - d6;      va <= 0 and g >= 0 and h >= 0: q = B + (g / (g + h)) (C - B)
 *      otherwise s = (va + vb) + vc: q = (A + (vb / s) ab) + (vc / s) ac.
 *    A distance that is a NaN (a degenerate face) takes no part in the minimum; the minimum of numbers is exact, its order is free.
 *    Depth is evaluated for inside vertices only.
 * 7. A frame of the unordered pair (a, b), a < b.  inside[0] = the vertices of a inside b, inside[1] = the vertices of b inside a;
 *    a CONTACT frame has inside[0] + inside[1] > 0.  depth = the maximum depth of these vertices over the total order (larger depth,
 *    then the lower dancer, then the lower vertex), 0 without contact.  An invalid frame reports inside = (-1, -1) and depth = NaN,
 *    is no contact frame, leaves the numerator and the denominator of every rate and changes nothing about other frames.
 * 8. Per clip and pair, in tcg pair order (0,1), (0,2), ..., (1,2), ..., P = dn (dn - 1) / 2, n = the valid frames:
 *    rate = contact frames / n (NaN if n == 0); episodes = the maximal runs of contact frames (an invalid frame ends a run);
 *    depth_max = the largest depth over the total order (larger depth, then lower frame, lower dancer, lower vertex), 0 without
 *    contact, and deepest = (frame, dancer whose vertex it is, vertex), (-1, -1, -1) without contact; inside_mean = (the sum over the
 *    valid frames of inside[0] + inside[1], an integer, so exact in any order) / n (NaN if n == 0).
 *
 * ---- the broad phase: it changes no result --------------------------------------------------------------------------------------
 * Each pose has an axis-aligned box in float32, the exact minimum and maximum of its components.  A crossed edge has
 * min(u.y, w.y) <= p.y <= max(u.y, w.y) and p.x < xe <= max(u.x, w.x) (the quotient lies in [0, 1] and float32 differences are exact
 * in float64), and a closed polygon is crossed an even number of times by a ray that starts left of all of it: a face can cover p
 * only if p.x and p.y lie in the face's floor-plane box.  z_hit lies between the face's heights up to float64 rounding, far less than
 * one float32 step, and every test below is an exact float32 compare that keeps the equal case.  So a vertex of a whose x or y lies
 * outside b's box, or whose z is above it, is not inside b, and a pair whose boxes are disjoint in x or y, or with a's box above b's,
 * has no vertex of a inside b; on a closed mesh the same holds for a vertex below b's box (every covering face is above it and
 * their signs cancel).  The kernels use the first set, which holds for an open mesh too.
 *
 * ---- the launchers (csrc/meshcontact.hip) -------------------------------------------------------------------------------------------
 * TC_MESH_LAUNCHES launches whatever b is; no atomics, counts are integers, every maximum is over the total order: the same input
 * gives the same bits.
 *   boxes:   one workgroup per pose: minimum and maximum over V and the finite flag, into the workspace.
 *   contact: one workgroup of TC_MESH_THREADS per (clip, frame, ordered pair); it leaves at once when the frame is invalid or the
 *            boxes rule contact out.  Otherwise a's vertices in chunks of TC_MESH_THREADS, those that pass the box test compacted by
 *            ballot and prefix into an LDS list of at most TC_MESH_CANDIDATES; b's faces in chunks, those whose floor-plane box
 *            meets the candidates' and that reach above the lowest candidate compacted into an LDS tile of at most TC_MESH_TILE
 *            faces, nine floats each; candidates x tile with a lane per candidate; the inside candidates compacted, and for those
 *            alone the distance pass over all faces, tile by tile, a wave per vertex, skipping a face whose box is further from the
 *            vertex than the nearest counted face above it (the vertex's depth is at most that; float32 with slack, it changes no
 *            result).  Writes count, depth and arg-max of its frame and direction into the workspace.
 *   reduce:  one workgroup per (clip, pair): the frames for the rate, the episodes, the mean and the arg-max, and the frame planes.
 * workspace: TC_MESH_WS_POSE bytes per pose (six floats of box, the flag, a pad) and TC_MESH_WS_ORDERED bytes per (clip, frame,
 *   ordered pair) (depth float64, count and vertex int32), aligned to 8.
 *
 * The checks, in this order.  TC_ERR_ARG: a NULL pointer (inside and depth may be NULL); b, dn, T, V or F < 1; up outside 0..2.
 * TC_ERR_UNSUPPORTED: more than 2^31 - 1 vertex components (b T dn V 3), face indices (3 F) or (clip, frame, ordered pair) triples.
 * TC_ERR_ARG: a negative stride; a face index below 0 or >= V (read from faces_host); workspace_bytes below
 * tcm_mesh_contact_workspace's.  TC_ERR_ALIGN: workspace or depth not aligned to 8 bytes, inside not to 4.  With dn == 1 there is no
 * pair: after the checks the call returns TC_OK and launches nothing.
 * tcm_mesh_contact_workspace: TC_ERR_ARG for a NULL `bytes`, the same shape checks, TC_ERR_UNSUPPORTED likewise. */
#ifndef TCDIFF_MESHCONTACT_H
#define TCDIFF_MESHCONTACT_H

#include "tcdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TC_MESH_LAUNCHES 3
#define TC_MESH_THREADS 256
#define TC_MESH_CANDIDATES 1024
#define TC_MESH_TILE 512
#define TC_MESH_WS_POSE 32
#define TC_MESH_WS_ORDERED 16

/* bytes[0] (a HOST long) = the workspace tcm_mesh_contact needs for b clips of T frames of dn dancers with V vertices and F faces */
int tcm_mesh_contact_workspace(int b, int dn, int T, int V, int F, long* bytes);

/* inside [b][P][T][2] int32 or NULL; depth [b][P][T] float64 or NULL; rate, depth_max, inside_mean [b P] float64; episodes [b P]
 * int64 (long); deepest [b P][3] int64. */
int tcm_mesh_contact(const float* vertices, const long* vertex_strides, const int* faces, const int* faces_host, int b, int dn, int T,
                     int V, int F, int up, void* workspace, long workspace_bytes, int* inside, double* depth, double* rate,
                     long* episodes, double* depth_max, long* deepest, double* inside_mean, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TCDIFF_MESHCONTACT_H */
