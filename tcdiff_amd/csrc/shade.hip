// Shaded, depth-tested frames of triangle meshes (the skinned SMPL bodies), gfx950: a small software rasteriser.  The picture's
// definition is in include/tcdiff_shade.h; tests/shade_ref.py restates it in numpy float64; the arithmetic is csrc/shade_math.h,
// which the tests also build for the host.
//
// shade_vertices_kernel: one thread per (pose, vertex): the screen position (the fmaf chain of draw_project_kernel) and the
//   area-weighted vertex normal, a float64 sum over the vertex's faces in the order the host's CSR adjacency lists them.
// shade_box_kernel: one workgroup per chunk of 256 consecutive triangles of one frame, one thread per triangle: gathers the three
//   screen vertices and writes the triangle's pixel box, clamped to the image in floating point before it becomes four integers
//   (8 bytes; an empty box for anything that is not finite or not indexable), and the chunk's box, the union of its 256 (wave
//   shuffles, then LDS over the four waves).
// shade_tile_kernel: grid (tiles, T, clips), one workgroup of 256 threads per 32 x 32 tile of one frame, four neighbouring pixels
//   of one row per thread.  Each wave reads 64 chunk boxes at a time and ballots the ones that meet the tile -- the same mask in all
//   four waves -- so a chunk that misses the tile costs no barrier (neighbouring faces of a body lie together: most chunks miss
//   most tiles).  A chunk that meets it is read whole (one coalesced 8-byte load per thread), the triangles whose
//   box meets the tile are compacted into LDS in ascending index (wave ballot + prefix over the four waves, as draw_raster_kernel)
//   and set up there by the thread that kept them.  Each wave then ballots, 64 kept triangles at a time, the ones that reach its 8
//   rows and visits those alone; a thread skips one that misses its four pixels; every other pixel evaluates the three edge functions in float64 and keeps the best
//   (z, g) and its weights in registers.  No atomics, no list in memory whose size would have to be guessed: a tile that holds
//   every triangle of the frame takes the same path as an empty one.  The winner is shaded once per pixel at the end.
#include "common.h"
#include "shade_math.h"
#include "tcdiff_shade.h"

#define TC_SHADE_THREADS 256
static_assert(TC_SHADE_CHUNK == TC_SHADE_THREADS, "one box per thread and chunk");
static_assert(TC_SHADE_TILE * TC_SHADE_TILE == 4 * TC_SHADE_THREADS, "four pixels per thread");
static_assert(TC_SHADE_SCRATCH_PER_TRIANGLE == sizeof(int2), "one packed box per triangle and per chunk");

struct shade_view {
    float m[12];
};

DEVINL float shade_proj(const float* __restrict__ m, float X, float Y, float Z) {
    return fmaf(m[2], Z, fmaf(m[1], Y, fmaf(m[0], X, m[3])));
}

__global__ __launch_bounds__(256) void shade_vertices_kernel(const float* __restrict__ vertices, const int* __restrict__ faces,
                                                             const int* __restrict__ adj_start, const int* __restrict__ adj_faces,
                                                             long n, int V, int F, shade_view view, float* __restrict__ screen,
                                                             float* __restrict__ normals) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;      // pose * V + vertex
    if (i >= n) return;
    const long pose = i / V;
    const int v = (int)(i - pose * V);
    const float* P = vertices + pose * V * 3;
    if (screen) {
        const float X = P[3 * v], Y = P[3 * v + 1], Z = P[3 * v + 2];
        screen[3 * i] = shade_proj(view.m, X, Y, Z);
        screen[3 * i + 1] = shade_proj(view.m + 4, X, Y, Z);
        screen[3 * i + 2] = shade_proj(view.m + 8, X, Y, Z);
    }
    if (!normals) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int lo = adj_start[v], hi = adj_start[v + 1];
    lo = max(lo, 0), hi = min(hi, 3 * F);                     // a range outside adj_faces is never read
    for (int k = lo; k < hi; ++k) {
        const int f = adj_faces[k];
        if ((unsigned)f >= (unsigned)F) continue;
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) continue;
        const float *p0 = P + 3 * i0, *p1 = P + 3 * i1, *p2 = P + 3 * i2;
        const double e1x = (double)p1[0] - (double)p0[0], e1y = (double)p1[1] - (double)p0[1], e1z = (double)p1[2] - (double)p0[2];
        const double e2x = (double)p2[0] - (double)p0[0], e2y = (double)p2[1] - (double)p0[1], e2z = (double)p2[2] - (double)p0[2];
        sx += e1y * e2z - e1z * e2y;
        sy += e1z * e2x - e1x * e2z;
        sz += e1x * e2y - e1y * e2x;
    }
    const double len = sqrt((sx * sx + sy * sy) + sz * sz);
    float* o = normals + 3 * i;
    if (len == 0.0) {
        o[0] = o[1] = o[2] = 0.f;
    } else {
        o[0] = (float)(sx / len), o[1] = (float)(sy / len), o[2] = (float)(sz / len);
    }
}

struct shade_args {
    const float* screen;
    const float* normals;
    const int* faces;
    const unsigned char* colors;
    const unsigned char* under;
    int2* boxes;                                          // [frames][G], then the chunks' boxes [frames][chunks]
    int2* chunk_boxes;
    unsigned char* frames;
    int dn, T, V, F, W, H, n_colors, tiles_x, vec;
    tcr_shade_style st;
};

// the three vertex indices of face f, or false when one is no vertex
DEVINL bool shade_face(const shade_args& A, int f, int* idx) {
    idx[0] = A.faces[3 * f], idx[1] = A.faces[3 * f + 1], idx[2] = A.faces[3 * f + 2];
    return (unsigned)idx[0] < (unsigned)A.V && (unsigned)idx[1] < (unsigned)A.V && (unsigned)idx[2] < (unsigned)A.V;
}

DEVINL int2 shade_pack(int x0, int x1, int y0, int y1) {
    return x0 <= x1 && y0 <= y1 ? make_int2(x0 | x1 << 16, y0 | y1 << 16) : make_int2(1, 1);      // the empty box: x0 = 1 > x1 = 0
}

__global__ __launch_bounds__(TC_SHADE_CHUNK) void shade_box_kernel(const shade_args A, int chunks) {
    __shared__ int s_part[TC_SHADE_CHUNK / TC_WAVE][4];
    const int tid = threadIdx.x, lane = tid & (TC_WAVE - 1), wave = tid / TC_WAVE;
    const long frame = blockIdx.x / chunks;
    const int chunk = (int)(blockIdx.x - frame * chunks);
    const int G = A.dn * A.F, g = chunk * TC_SHADE_CHUNK + tid;
    shade_box B;
    B.x0 = B.y0 = 1, B.x1 = B.y1 = 0;
    if (g < G) {
        const int d = g / A.F, f = g - d * A.F;
        int idx[3];
        if (shade_face(A, f, idx)) {
            const float* S = A.screen + (frame * A.dn + d) * A.V * 3;
            B = shade_make_box(S + 3 * idx[0], S + 3 * idx[1], S + 3 * idx[2], A.W, A.H);
        }
        A.boxes[frame * G + g] = shade_pack(B.x0, B.x1, B.y0, B.y1);
    }
    // the chunk's box: the union of the boxes that are not empty (an empty one joins with the neutral values)
    const bool some = B.x0 <= B.x1;
    int x0 = some ? B.x0 : 0x7fff, x1 = some ? B.x1 : -1, y0 = some ? B.y0 : 0x7fff, y1 = some ? B.y1 : -1;
#pragma unroll
    for (int off = TC_WAVE / 2; off > 0; off >>= 1) {
        x0 = min(x0, __shfl_xor(x0, off)), x1 = max(x1, __shfl_xor(x1, off));
        y0 = min(y0, __shfl_xor(y0, off)), y1 = max(y1, __shfl_xor(y1, off));
    }
    if (lane == 0) s_part[wave][0] = x0, s_part[wave][1] = x1, s_part[wave][2] = y0, s_part[wave][3] = y1;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < TC_SHADE_CHUNK / TC_WAVE; ++w) {
            x0 = min(x0, s_part[w][0]), x1 = max(x1, s_part[w][1]);
            y0 = min(y0, s_part[w][2]), y1 = max(y1, s_part[w][3]);
        }
        A.chunk_boxes[blockIdx.x] = shade_pack(x0, x1, y0, y1);
    }
}

__global__ __launch_bounds__(TC_SHADE_THREADS) void shade_tile_kernel(const shade_args A) {
#pragma clang fp contract(off)
    __shared__ shade_tri s_tri[TC_SHADE_CHUNK];
    __shared__ int2 s_box[TC_SHADE_CHUNK];
    __shared__ int s_g[TC_SHADE_CHUNK];
    __shared__ int s_wave[TC_SHADE_THREADS / TC_WAVE];
    const int tid = threadIdx.x, lane = tid & (TC_WAVE - 1), wave = __builtin_amdgcn_readfirstlane(tid / TC_WAVE);
    const int t = blockIdx.y;
    const long frame = (long)blockIdx.z * A.T + t;
    const int tile_y = blockIdx.x / A.tiles_x, tile_x = blockIdx.x - tile_y * A.tiles_x;
    const int x_lo = tile_x * TC_SHADE_TILE, y_lo = tile_y * TC_SHADE_TILE;
    const int x_hi = min(x_lo + TC_SHADE_TILE, A.W) - 1, y_hi = min(y_lo + TC_SHADE_TILE, A.H) - 1;      // the tile's pixels [lo, hi]
    const int x0 = x_lo + 4 * (tid & 7), y = y_lo + (tid >> 3);                                          // this thread's pixels x0 .. x0 + 3
    const int band_lo = y_lo + 8 * wave, band_hi = band_lo + 7;                                          // this wave's rows
    const double py = y + 0.5;
    const int G = A.dn * A.F;
    const int chunks = (G + TC_SHADE_CHUNK - 1) / TC_SHADE_CHUNK;
    const int2* boxes = A.boxes + frame * G;
    const int2* chunk_boxes = A.chunk_boxes + frame * chunks;
    const float* S = A.screen + frame * A.dn * A.V * 3;

    double best_z[4], w0[4], w1[4], w2[4];
    int best_g[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) best_z[p] = 0.0, w0[p] = w1[p] = w2[p] = 0.0, best_g[p] = -1;

    for (int first = 0; first < chunks; first += TC_WAVE) {
        // 64 chunk boxes per wave; every wave reads the same ones, so the mask, and with it every barrier below, is the workgroup's
        int meets = 0;
        if (first + lane < chunks) {
            const int2 u = chunk_boxes[first + lane];
            const int ux0 = u.x & 0xffff, ux1 = u.x >> 16, uy0 = u.y & 0xffff, uy1 = u.y >> 16;
            meets = ux0 <= ux1 && ux0 <= x_hi && ux1 >= x_lo && uy0 <= y_hi && uy1 >= y_lo;
        }
        for (unsigned long long todo = __ballot(meets); todo; todo &= todo - 1) {
            const int base = (first + __builtin_ctzll(todo)) * TC_SHADE_CHUNK;
            const int g = base + tid;
            int keep = 0;
            int2 box = make_int2(1, 1);
            if (g < G) {
                box = boxes[g];
                const int bx0 = box.x & 0xffff, bx1 = box.x >> 16, by0 = box.y & 0xffff, by1 = box.y >> 16;
                keep = bx0 <= bx1 && bx0 <= x_hi && bx1 >= x_lo && by0 <= y_hi && by1 >= y_lo;
            }
            const unsigned long long vote = __ballot(keep);
            if (lane == 0) s_wave[wave] = __popcll(vote);
            __syncthreads();                                  // (also: the previous chunk's list has been read)
            int pos = __popcll(vote & ((1ull << lane) - 1ull)), kept = 0;
#pragma unroll
            for (int w = 0; w < TC_SHADE_THREADS / TC_WAVE; ++w) {
                if (w < wave) pos += s_wave[w];
                kept += s_wave[w];
            }
            if (keep) {
                const int d = g / A.F, f = g - d * A.F;
                int idx[3];
                shade_face(A, f, idx);                        // a kept box is not empty: the indices were in range when it was made
                const float* Sd = S + (long)d * A.V * 3;
                s_tri[pos] = shade_setup(Sd + 3 * idx[0], Sd + 3 * idx[1], Sd + 3 * idx[2]);
                s_box[pos] = box;
                s_g[pos] = g;
            }
            __syncthreads();
            kept = __builtin_amdgcn_readfirstlane(kept);
            for (int j0 = 0; j0 < kept; j0 += TC_WAVE) {
                // 64 kept triangles per step, one per lane: the ones that reach this wave's eight rows, then those alone, in order
                int reaches = 0;
                if (j0 + lane < kept) {
                    const int2 b = s_box[j0 + lane];
                    reaches = (b.y & 0xffff) <= band_hi && (b.y >> 16) >= band_lo;
                }
                for (unsigned long long mine = __ballot(reaches); mine; mine &= mine - 1) {
                    const int j = j0 + __builtin_ctzll(mine);
                    const int2 b = s_box[j];
                    const int bx0 = b.x & 0xffff, bx1 = b.x >> 16, by0 = b.y & 0xffff, by1 = b.y >> 16;
                    if (y < by0 || y > by1 || x0 > bx1 || x0 + 3 < bx0) continue;
                    const shade_tri& tri = s_tri[j];
                    const int gj = s_g[j];
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int x = x0 + p;
                        if (x < bx0 || x > bx1) continue;
                        double E[3], area;
                        if (!shade_edges(tri, x + 0.5, py, E, &area)) continue;
                        const double z = shade_depth(tri, E, area);
                        if (best_g[p] < 0 || z < best_z[p] || (z == best_z[p] && gj < best_g[p])) {
                            best_z[p] = z, best_g[p] = gj;
                            w0[p] = E[0], w1[p] = E[1], w2[p] = E[2];
                        }
                    }
                }
            }
            // the next chunk's first barrier keeps its writes behind these reads
        }
    }

    if (y > y_hi) return;
    const long row_off = ((frame * A.H + y) * (long)A.W) * 3;
    unsigned char out[12];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int x = x0 + p;
        if (best_g[p] >= 0) {
            const int d = best_g[p] / A.F, f = best_g[p] - d * A.F;
            int idx[3];
            shade_face(A, f, idx);
            const float* N = A.normals + (frame * A.dn + d) * A.V * 3;
            const double E[3] = {w0[p], w1[p], w2[p]};
            const double k = shade_factor(N + 3 * idx[0], N + 3 * idx[1], N + 3 * idx[2], E, A.st.light, (double)A.st.ambient);
            const unsigned char* col = A.colors + 3 * (d % A.n_colors);
#pragma unroll
            for (int c = 0; c < 3; ++c) out[3 * p + c] = shade_level(col[c], k);
        } else if (A.under && x <= x_hi) {
#pragma unroll
            for (int c = 0; c < 3; ++c) out[3 * p + c] = A.under[row_off + 3L * x + c];
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) out[3 * p + c] = A.st.background[c];
        }
    }
    unsigned char* row = A.frames + row_off;
    if (A.vec && x0 + 3 < A.W) {                          // 12 bytes on a 4-byte boundary: three dword stores
        unsigned* o = reinterpret_cast<unsigned*>(row + 3L * x0);
#pragma unroll
        for (int w = 0; w < 3; ++w)
            o[w] = (unsigned)out[4 * w] | (unsigned)out[4 * w + 1] << 8 | (unsigned)out[4 * w + 2] << 16 | (unsigned)out[4 * w + 3] << 24;
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (x0 + p < A.W) {
                row[3L * (x0 + p)] = out[3 * p];
                row[3L * (x0 + p) + 1] = out[3 * p + 1];
                row[3L * (x0 + p) + 2] = out[3 * p + 2];
            }
    }
}

extern "C" int tcr_mesh_vertices(const float* vertices, const int* faces, const int* adj_start, const int* adj_faces, int P, int V, int F,
                                 const float* view, float* screen, float* normals, hipStream_t stream) {
    if (!vertices || !faces || !view || (!screen && !normals)) return TC_ERR_ARG;
    if (normals && (!adj_start || !adj_faces)) return TC_ERR_ARG;
    if (P < 1 || V < 1 || F < 1) return TC_ERR_ARG;
    if ((long)P * V > 0x7fffffffL / 3 || (long)F > 0x7fffffffL / 3) return TC_ERR_UNSUPPORTED;
    shade_view v;
    for (int i = 0; i < 12; ++i) v.m[i] = view[i];
    const long n = (long)P * V;
    hipLaunchKernelGGL(shade_vertices_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, vertices, faces, adj_start,
                       adj_faces, n, V, F, v, screen, normals);
    TC_CHECK_LAUNCH();
    return TC_OK;
}

extern "C" int tcr_mesh_raster(const float* screen, const float* normals, const int* faces, int b, int T, int dn, int V, int F, int W,
                               int H, const unsigned char* colors, int n_colors, const tcr_shade_style* style, const unsigned char* under,
                               int* scratch, long scratch_bytes, unsigned char* frames, hipStream_t stream) {
    if (!screen || !normals || !faces || !colors || !style || !scratch || !frames) return TC_ERR_ARG;
    if (b < 1 || T < 1 || dn < 1 || V < 1 || F < 1 || W < 1 || H < 1 || n_colors < 1) return TC_ERR_ARG;
    if (!(style->ambient >= 0.f && style->ambient <= 1.f)) return TC_ERR_ARG;
    double l2 = 0.0;
    for (int i = 0; i < 3; ++i) {
        if (!(fabsf(style->light[i]) < __builtin_inff())) return TC_ERR_ARG;
        l2 += (double)style->light[i] * (double)style->light[i];
    }
    if (!(fabs(l2 - 1.0) <= 1e-3)) return TC_ERR_ARG;
    if (b > 65535 || T > 65535 || W > TC_SHADE_MAX_SIDE || H > TC_SHADE_MAX_SIDE) return TC_ERR_UNSUPPORTED;
    const long lim = 0x7fffffffL, poses = (long)b * T * dn;                    // b T <= 2^32: no product below overflows a long
    if (poses > lim || poses * V > lim / 3 || poses * F > lim || (long)b * T * H > lim || (long)b * T * H * W > lim / 3)
        return TC_ERR_UNSUPPORTED;
    const long n = poses * F, frames_n = (long)b * T;
    const int chunks = (int)(((long)dn * F + TC_SHADE_CHUNK - 1) / TC_SHADE_CHUNK);          // per frame
    if (scratch_bytes < TC_SHADE_SCRATCH_PER_TRIANGLE * (n + frames_n * chunks)) return TC_ERR_ARG;
    if ((uintptr_t)scratch % 8 != 0) return TC_ERR_ALIGN;
    const int tiles_x = (W + TC_SHADE_TILE - 1) / TC_SHADE_TILE, tiles_y = (H + TC_SHADE_TILE - 1) / TC_SHADE_TILE;
    shade_args A;
    A.screen = screen, A.normals = normals, A.faces = faces, A.colors = colors, A.under = under;
    A.boxes = reinterpret_cast<int2*>(scratch), A.chunk_boxes = A.boxes + n, A.frames = frames;
    A.dn = dn, A.T = T, A.V = V, A.F = F, A.W = W, A.H = H, A.n_colors = n_colors, A.tiles_x = tiles_x;
    A.vec = (W % 4 == 0 && (uintptr_t)frames % 4 == 0) ? 1 : 0;
    A.st = *style;
    hipLaunchKernelGGL(shade_box_kernel, dim3((unsigned)(frames_n * chunks)), dim3(TC_SHADE_CHUNK), 0, stream, A, chunks);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(shade_tile_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)T, (unsigned)b), dim3(TC_SHADE_THREADS), 0,
                       stream, A);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
