// Stick-figure frames of generated group dances, gfx950: what the reference's skeleton_render (vis.py:223-327) draws with
// matplotlib on the host, one FuncAnimation frame at a time, as a small software rasteriser.  Two launches for any number of
// clips, no host synchronisation, no atomics, a fixed paint order: same input, same bits.  The picture's definition is in
// include/tcdiff_hip.h; tests/draw_ref.py restates it in numpy float64.
//
// draw_project_kernel: one workgroup per (clip, frame).  Reads joints / contacts in place through their element strides,
//   projects every joint and the floor trail point with one fmaf chain per screen coordinate (float32, three roundings),
//   decides which feet are planted (float64 on the float32 inputs, as csrc/metrics.hip) and ranks the dancers far to near.
//   The ranks are counted from depths every thread recomputes with the same chain, so nothing is read back from memory.
// draw_raster_kernel: grid (tiles, T, clips), one workgroup of 256 threads per 32 x 32 tile of one frame, four neighbouring
//   pixels of one row per thread.  The frame's primitives are enumerated in paint order, 256 at a time (one per thread):
//   each thread builds its primitive, tests its inflated bounding box against the tile, and the survivors are compacted
//   into LDS in paint order (wave ballot + prefix over the four waves).  Every pixel then blends the kept list, and the
//   next chunk follows, so a frame of any number of primitives takes the same path with a fixed amount of LDS.  Per-pixel
//   arithmetic is float64: a blend is then good to ~1e-8 levels, far below the rounding to a byte, and the test can ask for
//   equal bytes on all but the pixels that sit on a rounding boundary.
#include "common.h"
#include "tcdiff_hip.h"

#define TC_DRAW_THREADS 256
#define TC_DRAW_TILE 32
#define TC_DRAW_CULL_MARGIN 0.015625                      // 1 / 64 pixel: far above the error of a computed distance

struct draw_view {
    float m[12];
};

// row . (X, Y, Z, 1): three fused multiply-adds, so at most 3 * 2^-24 * (|m0 X| + |m1 Y| + |m2 Z| + |m3|) from the exact value
DEVINL float draw_proj(const float* __restrict__ m, float X, float Y, float Z) {
    return fmaf(m[2], Z, fmaf(m[1], Y, fmaf(m[0], X, m[3])));
}

DEVINL float draw_depth_key(float z) { return z == z ? z : __builtin_inff(); }      // a NaN depth counts as the farthest

__global__ __launch_bounds__(64) void draw_project_kernel(const float* __restrict__ joints, long jsb, long jsd, long jst,
                                                         const float* __restrict__ contacts, long csb, long csd, long cst, int dn,
                                                         int T, draw_view view, float floor, int up, double thr, double still,
                                                         float* __restrict__ pts, float* __restrict__ trail, int* __restrict__ order,
                                                         unsigned char* __restrict__ planted) {
#pragma clang fp contract(off)
    const long f = blockIdx.x;                            // clip * T + frame
    const long c = f / T;
    const int t = (int)(f - c * T);
    const int tid = threadIdx.x;
    const float* J = joints + c * jsb + (long)t * jst;
    for (int i = tid; i < dn * 24; i += 64) {
        const int d = i / 24, j = i - d * 24;
        const float* p = J + d * jsd + 3 * j;
        float* o = pts + ((f * dn + d) * 24 + j) * 3;
        o[0] = draw_proj(view.m, p[0], p[1], p[2]);
        o[1] = draw_proj(view.m + 4, p[0], p[1], p[2]);
        o[2] = draw_proj(view.m + 8, p[0], p[1], p[2]);
    }
    for (int d = tid; d < dn; d += 64) {
        const float* p = J + d * jsd;
        const float X = up == 0 ? floor : p[0], Y = up == 1 ? floor : p[1], Z = up == 2 ? floor : p[2];
        float* o = trail + (f * dn + d) * 2;
        o[0] = draw_proj(view.m, X, Y, Z);
        o[1] = draw_proj(view.m + 4, X, Y, Z);
        // painter's rank: the dancers that are drawn before d
        const float zd = draw_depth_key(draw_proj(view.m + 8, p[0], p[1], p[2]));
        int rank = 0;
        for (int e = 0; e < dn; ++e) {
            const float* q = J + e * jsd;
            const float ze = draw_depth_key(draw_proj(view.m + 8, q[0], q[1], q[2]));
            rank += (ze > zd || (ze == zd && e < d)) ? 1 : 0;
        }
        order[f * dn + rank] = d;
    }
    for (int i = tid; i < dn * 4; i += 64) {
        const int d = i >> 2, k = i & 3;
        const int foot = k == 0 ? 7 : k == 1 ? 8 : k == 2 ? 10 : 11;
        int on;
        if (contacts) {
            on = (double)contacts[c * csb + d * csd + (long)t * cst + k] > thr;
        } else if (t + 1 < T) {
            const float* p = J + d * jsd + 3 * foot;
            const float* q = p + jst;
            const double dx = (double)q[0] - (double)p[0], dy = (double)q[1] - (double)p[1], dz = (double)q[2] - (double)p[2];
            on = sqrt(dx * dx + dy * dy + dz * dz) < still;
        } else {
            on = 1;
        }
        planted[(f * dn + d) * 4 + k] = (unsigned char)on;
    }
}

struct draw_prim {
    float ax, ay, bx, by, hw, alpha;
    unsigned rgb;
};

struct draw_raster_args {
    const float* pts;
    const float* trail;
    const int* order;
    const unsigned char* planted;
    const float* static_segs;
    const unsigned char* colors;
    unsigned char* frames;
    int dn, T, W, H, n_static, n_colors, tiles_x, vec;
    int parents[24];
    tcdiff_draw_style st;
};

DEVINL unsigned draw_rgb(const unsigned char* p) { return (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16; }

// primitive i of frame (c, t) in paint order: static segments, trails by dancer index, bodies by painter's order
DEVINL draw_prim draw_make_prim(const draw_raster_args& A, long c, int t, int i, int t0, int nt, int per) {
    draw_prim P;
    P.ax = P.ay = P.bx = P.by = 0.f;
    P.hw = 0.f;
    P.alpha = 0.f;                                        // alpha 0: not drawn
    P.rgb = 0;
    const long f = c * A.T + t;
    if (i < A.n_static) {
        const float* s = A.static_segs + 4L * i;
        P.ax = s[0], P.ay = s[1], P.bx = s[2], P.by = s[3];
        P.hw = A.st.static_hw;
        P.alpha = A.st.static_alpha;
        P.rgb = draw_rgb(A.st.static_rgb);
        return P;
    }
    i -= A.n_static;
    if (i < A.dn * nt) {
        const int d = i / nt, tp = t0 + (i - d * nt);     // segment trail[tp - 1] -> trail[tp], 1 <= tp <= t
        const float* a = A.trail + ((c * A.T + tp - 1) * A.dn + d) * 2;
        const float* b = a + 2L * A.dn;
        P.ax = a[0], P.ay = a[1], P.bx = b[0], P.by = b[1];
        P.hw = A.st.trail_hw;
        P.alpha = A.st.trail_alpha;
        P.rgb = draw_rgb(A.colors + 3 * (d % A.n_colors));
        return P;
    }
    i -= A.dn * nt;
    const int r = i / per, k = i - r * per;
    const int d = A.order[f * A.dn + r];
    if (d < 0 || d >= A.dn) return P;                     // not a dancer: nothing is read through it
    const float* J = A.pts + (f * A.dn + d) * 72;
    if (k < 23) {
        const float* a = J + 3 * (k + 1);
        const float* b = J + 3 * A.parents[k + 1];
        P.ax = a[0], P.ay = a[1], P.bx = b[0], P.by = b[1];
        P.hw = A.st.line_hw;
        P.alpha = 1.f;
        P.rgb = draw_rgb(A.colors + 3 * (d % A.n_colors));
    } else {
        const int m = k - 23;
        const int foot = m == 0 ? 7 : m == 1 ? 8 : m == 2 ? 10 : 11;
        const float* a = J + 3 * foot;
        P.ax = P.bx = a[0], P.ay = P.by = a[1];
        P.hw = A.st.marker_radius;
        P.alpha = 1.f;
        P.rgb = draw_rgb(A.planted[(f * A.dn + d) * 4 + m] ? A.st.planted_rgb : A.st.free_rgb);
    }
    return P;
}

__global__ __launch_bounds__(TC_DRAW_THREADS) void draw_raster_kernel(const draw_raster_args A) {
#pragma clang fp contract(off)
    __shared__ double s_ax[TC_DRAW_THREADS], s_ay[TC_DRAW_THREADS], s_dx[TC_DRAW_THREADS], s_dy[TC_DRAW_THREADS];
    __shared__ double s_inv[TC_DRAW_THREADS], s_r[TC_DRAW_THREADS], s_alpha[TC_DRAW_THREADS];
    __shared__ unsigned s_rgb[TC_DRAW_THREADS];
    __shared__ int s_wave[TC_DRAW_THREADS / TC_WAVE];
    const int tid = threadIdx.x, lane = tid & (TC_WAVE - 1), wave = tid / TC_WAVE;
    const int t = blockIdx.y;
    const long c = blockIdx.z;
    const int tile_y = blockIdx.x / A.tiles_x, tile_x = blockIdx.x - tile_y * A.tiles_x;
    const int x_lo = tile_x * TC_DRAW_TILE, y_lo = tile_y * TC_DRAW_TILE;
    const int x_hi = min(x_lo + TC_DRAW_TILE, A.W), y_hi = min(y_lo + TC_DRAW_TILE, A.H);      // the tile's pixels [lo, hi)
    // the pixel centres the tile holds, widened by the margin
    const double cx_lo = x_lo + 0.5 - TC_DRAW_CULL_MARGIN, cx_hi = x_hi - 0.5 + TC_DRAW_CULL_MARGIN;
    const double cy_lo = y_lo + 0.5 - TC_DRAW_CULL_MARGIN, cy_hi = y_hi - 0.5 + TC_DRAW_CULL_MARGIN;
    const int x0 = x_lo + 4 * (tid & 7), y = y_lo + (tid >> 3);                                // this thread's pixels x0 .. x0 + 3
    const double py = y + 0.5;

    double col[4][3];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int k = 0; k < 3; ++k) col[p][k] = (double)A.st.background[k];

    const int t0 = A.st.trail_len <= 0 ? 1 : max(1, t - A.st.trail_len + 1);
    const int nt = t >= t0 ? t - t0 + 1 : 0;
    const int per = 23 + (A.st.markers ? 4 : 0);
    const int n = A.n_static + A.dn * nt + A.dn * per;

    for (int base = 0; base < n; base += TC_DRAW_THREADS) {
        const int i = base + tid;
        int keep = 0;
        draw_prim P;
        if (i < n) {
            P = draw_make_prim(A, c, t, i, t0, nt, per);
            const bool finite = fabsf(P.ax) < __builtin_inff() && fabsf(P.ay) < __builtin_inff() &&
                                fabsf(P.bx) < __builtin_inff() && fabsf(P.by) < __builtin_inff();
            const double r = (double)P.hw + 0.5;
            // coverage is 0 wherever the distance to the segment is >= r, so it is 0 on the whole tile when the segment's
            // bounding box, grown by r, misses the tile's pixel centres
            keep = finite && P.alpha > 0.f && (double)fminf(P.ax, P.bx) - r <= cx_hi && (double)fmaxf(P.ax, P.bx) + r >= cx_lo &&
                   (double)fminf(P.ay, P.by) - r <= cy_hi && (double)fmaxf(P.ay, P.by) + r >= cy_lo;
        }
        const unsigned long long vote = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(vote);
        __syncthreads();                                  // (also: the previous chunk's list has been read)
        int pos = __popcll(vote & ((1ull << lane) - 1ull)), kept = 0;
#pragma unroll
        for (int w = 0; w < TC_DRAW_THREADS / TC_WAVE; ++w) {
            if (w < wave) pos += s_wave[w];
            kept += s_wave[w];
        }
        if (keep) {
            const double dx = (double)P.bx - (double)P.ax, dy = (double)P.by - (double)P.ay;
            const double len2 = dx * dx + dy * dy;
            s_ax[pos] = P.ax, s_ay[pos] = P.ay, s_dx[pos] = dx, s_dy[pos] = dy;
            s_inv[pos] = len2 > 0.0 ? 1.0 / len2 : 0.0;   // a segment of zero length is a disc: parameter 0
            s_r[pos] = (double)P.hw + 0.5;
            s_alpha[pos] = P.alpha;
            s_rgb[pos] = P.rgb;
        }
        __syncthreads();
        for (int j = 0; j < kept; ++j) {
            const double ax = s_ax[j], ay = s_ay[j], dx = s_dx[j], dy = s_dy[j], inv = s_inv[j], r = s_r[j], alpha = s_alpha[j];
            const unsigned rgb = s_rgb[j];
            const double src[3] = {(double)(rgb & 255u), (double)(rgb >> 8 & 255u), (double)(rgb >> 16 & 255u)};
            const double ey = py - ay;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const double ex = (x0 + p) + 0.5 - ax;
                double u = (ex * dx + ey * dy) * inv;
                u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
                const double qx = ex - u * dx, qy = ey - u * dy;
                double cov = r - sqrt(qx * qx + qy * qy);
                if (cov > 0.0) {
                    cov = (cov > 1.0 ? 1.0 : cov) * alpha;
#pragma unroll
                    for (int k = 0; k < 3; ++k) col[p][k] += cov * (src[k] - col[p][k]);
                }
            }
        }
        // the next chunk's first barrier keeps its writes behind these reads
    }

    if (y >= y_hi) return;
    unsigned char out[12];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double v = col[p][k];
            v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
            out[3 * p + k] = (unsigned char)(v + 0.5);
        }
    unsigned char* row = A.frames + (((c * A.T + t) * A.H + y) * (long)A.W) * 3;
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

extern "C" int tcdiff_draw_project(const float* joints, const long* joint_strides, const float* contacts, const long* contact_strides,
                                   int b, int dn, int T, const float* view, float floor, int up, double contact_threshold,
                                   double still, float* pts, float* trail, int* order, unsigned char* planted, hipStream_t stream) {
    if (!joints || !joint_strides || !view || !pts || !trail || !order || !planted) return TC_ERR_ARG;
    if (contacts && !contact_strides) return TC_ERR_ARG;
    if (b < 1 || dn < 1 || T < 1 || up < 0 || up > 2) return TC_ERR_ARG;
    if ((long)b * T > 0x7fffffffL || (long)dn * 24 > 0x7fffffffL) return TC_ERR_UNSUPPORTED;
    draw_view v;
    for (int i = 0; i < 12; ++i) v.m[i] = view[i];
    const long cs[3] = {contacts ? contact_strides[0] : 0, contacts ? contact_strides[1] : 0, contacts ? contact_strides[2] : 0};
    hipLaunchKernelGGL(draw_project_kernel, dim3((unsigned)((long)b * T)), dim3(64), 0, stream, joints, joint_strides[0],
                       joint_strides[1], joint_strides[2], contacts, cs[0], cs[1], cs[2], dn, T, v, floor, up, contact_threshold, still,
                       pts, trail, order, planted);
    TC_CHECK_LAUNCH();
    return TC_OK;
}

extern "C" int tcdiff_draw_raster(const float* pts, const float* trail, const int* order, const unsigned char* planted, int b, int dn,
                                  int T, int W, int H, const int* parents, const float* static_segs, int n_static,
                                  const unsigned char* colors, int n_colors, const tcdiff_draw_style* style, unsigned char* frames,
                                  hipStream_t stream) {
    if (!pts || !trail || !order || !planted || !parents || !colors || !style || !frames) return TC_ERR_ARG;
    if (n_static < 0 || (n_static > 0 && !static_segs)) return TC_ERR_ARG;
    if (b < 1 || dn < 1 || T < 1 || W < 1 || H < 1 || n_colors < 1) return TC_ERR_ARG;
    for (int i = 1; i < 24; ++i)
        if (parents[i] < 0 || parents[i] >= 24) return TC_ERR_ARG;
    const float w[4] = {style->static_hw, style->line_hw, style->trail_hw, style->marker_radius};
    for (int i = 0; i < 4; ++i)
        if (!(w[i] >= 0.f && w[i] <= 16384.f)) return TC_ERR_ARG;
    if (!(style->static_alpha >= 0.f && style->static_alpha <= 1.f) || !(style->trail_alpha >= 0.f && style->trail_alpha <= 1.f))
        return TC_ERR_ARG;
    const long tiles_x = (W + TC_DRAW_TILE - 1) / TC_DRAW_TILE, tiles_y = (H + TC_DRAW_TILE - 1) / TC_DRAW_TILE;
    if (tiles_x * tiles_y > 0x7fffffffL || T > 65535 || b > 65535) return TC_ERR_UNSUPPORTED;
    if ((long)n_static + (long)dn * ((long)T + 27) > 0x7fffffffL - TC_DRAW_THREADS) return TC_ERR_UNSUPPORTED;
    draw_raster_args A;
    A.pts = pts, A.trail = trail, A.order = order, A.planted = planted, A.static_segs = static_segs, A.colors = colors;
    A.frames = frames;
    A.dn = dn, A.T = T, A.W = W, A.H = H, A.n_static = n_static, A.n_colors = n_colors, A.tiles_x = (int)tiles_x;
    A.vec = (W % 4 == 0 && (uintptr_t)frames % 4 == 0) ? 1 : 0;
    A.parents[0] = 0;
    for (int i = 1; i < 24; ++i) A.parents[i] = parents[i];
    A.st = *style;
    hipLaunchKernelGGL(draw_raster_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)T, (unsigned)b), dim3(TC_DRAW_THREADS), 0,
                       stream, A);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
