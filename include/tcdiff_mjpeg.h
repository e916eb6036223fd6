/* tcdiff_mjpeg.h -- the sixth header of libtcdiff_gfx950.so's C ABI: baseline JPEG frames encoded on the device, the video stream
 * of a Motion-JPEG AVI (tcdiff_amd/video.py packs the container on the host).  The conventions of tcdiff_hip.h hold: every function
 * returns 0 or a negative TC_ERR_* code, nothing is allocated, nothing synchronises the host, pointers are caller-owned DEVICE
 * pointers (`strides` and `bytes` excepted), work is enqueued on `stream`, the checks precede any GPU call.
 *
 * Why the functions are tcj_*: the sets of tcdiff_*, tcx_*, tcs_* and tcr_* symbols the library exports are frozen (the tests hold
 * each equal to the built library's dynamic symbols).  This header takes a prefix of its own; tcdiff_amd/_lib.py binds it as MJPEG
 * next to ABI, EXT, GLTF, SKIN and SHADE and adds it to none of them nor to EXPORTS.
 *
 * What follows is the definition of the bytes, and it is exact: the whole encoder is integer arithmetic, so csrc/mjpeg.hip, the
 * host build of csrc/mjpeg_math.h and the numpy restatement tests/mjpeg_ref.py give the SAME bytes.  Parity with another encoder's
 * bytes is unpinned; any baseline JPEG decoder reads the frames (the tests hold them to libjpeg through Pillow).  Not built:
 * progressive and optimised Huffman, 4:2:2, rate control.
 *
 * ---- input ----------------------------------------------------------------------------------------------------------------------
 * frames [N][H][W][3] uint8 RGB, read in place: pixel (n, y, x) is the three bytes at frames + n strides[0] + y strides[1] +
 * x strides[2] (element = byte strides, each >= 0; only the trailing 3 are contiguous).  1 <= W, H <= TC_MJPEG_MAX_SIDE.
 *
 * ---- colour: JFIF full-range YCbCr, 16-bit fixed point, round to nearest, then clamp to 0 .. 255 -----------------------------------
 *   Y  = ( 19595 R + 38470 G +  7471 B           + 32768) >> 16                (19595 + 38470 + 7471 = 65536)
 *   Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32768) >> 16                (the row sums to 0; 8388608 = 128 << 16)
 *   Cr = ( 32768 R - 27439 G -  5329 B + 8388608 + 32768) >> 16                (the row sums to 0)
 * Every sum is >= 0, so the shift is a plain division.  Cb and Cr reach 256 and are clamped to 255.  R = G = B = v gives Y = v,
 * Cb = Cr = 128.
 *
 * ---- subsampling ------------------------------------------------------------------------------------------------------------------
 * The image is padded to whole MCUs by repeating its last column and row: padded pixel (y, x) is pixel (min(y, H - 1), min(x, W - 1)).
 *   TC_MJPEG_444: MCU 8 x 8, blocks Y, Cb, Cr.
 *   TC_MJPEG_420: MCU 16 x 16, four Y blocks in raster order, then Cb, then Cr; a chroma sample is (a + b + c + d + 2) >> 2 of the
 *                 Cb (Cr) values, each rounded and clamped as above, of the 2 x 2 padded pixels it covers.
 * SOF0 carries the true W and H.
 *
 * ---- DCT ------------------------------------------------------------------------------------------------------------------------
 * s = sample - 128.  M[k][n] = round(s_k cos((2 n + 1) k pi / 16) 2^TC_MJPEG_DCT_BITS), s_0 = sqrt(1 / 8), s_k = 1 / 2, round half
 * away from zero (no entry is a tie), B = TC_MJPEG_DCT_BITS = 14:
 *   row 0:   5793   5793   5793   5793   5793   5793   5793   5793
 *   row 1:   8035   6811   4551   1598  -1598  -4551  -6811  -8035
 *   row 2:   7568   3135  -3135  -7568  -7568  -3135   3135   7568
 *   row 3:   6811  -1598  -8035  -4551   4551   8035   1598  -6811
 *   row 4:   5793  -5793  -5793   5793   5793  -5793  -5793   5793
 *   row 5:   4551  -8035   1598   6811  -6811  -1598   8035  -4551
 *   row 6:   3135  -7568   7568  -3135  -3135   7568  -7568   3135
 *   row 7:   1598  -4551   6811  -8035   8035  -6811   4551  -1598
 *   pass 1 (along x):  t[y][u] = (sum_n M[u][n] s[y][n] + 128) >> 8        an arithmetic shift (floor); t has 6 fractional bits
 *   pass 2 (along y):  c[v][u] =  sum_m M[v][m] t[m][u]                     c has TC_MJPEG_COEF_BITS = 20 fractional bits
 * int32 suffices: a row of M has sum |M| <= sqrt(8) 2^14 + 4 < 46346 (Cauchy-Schwarz on an orthonormal row, plus the roundings),
 * |s| <= 128, so the pass-1 sum is below 46346 * 128 < 2^23, |t| <= 23173, the pass-2 sum is below 46346 * 23173 < 1.08e9 < 2^31.
 * The coefficient goes into the quantiser with its 20 fractional bits; it is not rounded to an integer first.
 *
 * The bound on |c / 2^20 - float64 DCT|, in units of one coefficient.  An entry of M is off by at most 1/2, so pass 1 is off by
 * 8 * (1/2) * 128 / 2^14 = 2^-5 before its shift and by 2^-5 + 2^-7 after it (half a unit of 2^-6): e1 = 0.0390625.  The exact
 * 1-D transform T obeys |T| <= 128 sqrt(8), so |t| <= 64 (128 sqrt(8) + e1) < 23173.  Pass 2 is off by 8 * (1/2) * 23173 / 2^20
 * = 0.0884 for M's rounding, and by sqrt(8) e1 = 0.1105 for what pass 1 handed it: together below
 *   TC_MJPEG_DCT_BOUND_MILLI / 1000 = 0.2 of one coefficient.
 *
 * ---- quantisation ---------------------------------------------------------------------------------------------------------------
 * Annex K's base tables (K.1 luminance for Y, K.2 chrominance for Cb and Cr), scaled by the IJG rule: scale = 5000 / q (integer
 * division) for q < 50, else 200 - 2 q;  t = clamp((base * scale + 50) / 100, 1, 255), integer division;  q = quality in 1 .. 100.
 *   value = sign(c) * ((|c| + (t << 19)) / (t << 20))        round to nearest, ties away from zero; int32: 1.08e9 + 255 * 2^19 < 2^31
 * Then an AC value is clamped to +-1023, and the DC difference (below) to +-2047, so that no category appears that the standard
 * Huffman tables lack, whatever the rounding or the table.
 *
 * ---- entropy coding ---------------------------------------------------------------------------------------------------------------
 * Annex K.3's four standard Huffman tables (K.3 / K.4 DC, K.5 / K.6 AC; the luminance pair for Y, the chrominance pair for Cb, Cr),
 * codes assigned as Annex C does.  Per block, in zigzag order: the DC difference d = DC - pred, pred = the DC of the previous
 * block of the same component in the scan, 0 at the start of every restart interval (pred is the unclamped quantised DC), coded as
 * its category s (the number of bits of |d|) and then s amplitude bits: d for d > 0, d - 1 in s bits (one's complement) for d < 0.
 * Then for every non-zero AC value, with r the zeros since the previous one: r / 16 times ZRL (0xF0), then the symbol
 * ((r % 16) << 4) | s and s amplitude bits.  EOB (0x00) follows iff the block ends in zeros, i.e. iff coefficient 63 is zero.
 *
 * ---- the stream of one frame --------------------------------------------------------------------------------------------------------
 * TC_MJPEG_HEADER_BYTES = 625 bytes of segments, in this order, every length big-endian:
 *   SOI   FF D8
 *   APP0  FF E0 00 10 'J' 'F' 'I' 'F' 00  01 01  00  00 01 00 01  00 00               (1.01, density 1:1, no thumbnail)
 *   DQT   FF DB 00 84  00 <64 luminance values in zigzag order>  01 <64 chrominance values in zigzag order>
 *   SOF0  FF C0 00 11 08 H(2) W(2) 03   01 SS 00   02 11 01   03 11 01             SS = 22 (4:2:0) or 11 (4:4:4)
 *   DHT   FF C4 00 1F 00 <16 counts, 12 values>      DC luminance        DHT  FF C4 00 B5 10 <16 counts, 162 values>  AC luminance
 *   DHT   FF C4 00 1F 01 <16 counts, 12 values>      DC chrominance      DHT  FF C4 00 B5 11 <16 counts, 162 values>  AC chrominance
 *   DRI   FF DD 00 04 Ri(2)                 Ri = the MCUs of one MCU row = ceil(W / 8) or ceil(W / 16)
 *   SOS   FF DA 00 0C 03  01 00  02 11  03 11  00 3F 00                              one interleaved scan
 * then the entropy data and EOI (FF D9).  THE RESTART INTERVAL IS ONE MCU ROW: intervals are byte-aligned and independent, which
 * is the grain of the encoder's parallelism.  Each interval is padded to a whole byte with 1-bits; every 0xFF byte of an
 * interval's data (padding included) is followed by 0x00; between interval i and i + 1 sits RSTm = FF D0+m, m = i % 8.
 *
 * ---- the launchers (csrc/mjpeg.hip) ---------------------------------------------------------------------------------------------------
 * Two calls with one scalar read-back between them (offsets[N], so that `data` is allocated exactly); no frame bytes cross to the
 * host.  TC_MJPEG_LAUNCHES launches in all, whatever N is:
 *   plan  1. blocks: one wave per 8 x 8 block -- gather through the strides, convert, downsample, transform through LDS, quantise;
 *            writes the zigzag-ordered int16 coefficients and the bit length of the block's AC symbols (wave ballot: a non-zero
 *            lane finds its run in the mask).
 *         2. count: one workgroup of TC_MJPEG_THREADS threads per interval (frame, MCU row), looping when the interval holds more
 *            blocks than threads -- DC differences, a workgroup scan of the bit lengths (each block's bit offset replaces its
 *            length), then the interval is packed in LDS in windows of TC_MJPEG_WINDOW bytes to count its 0xFF bytes: the
 *            interval's exact byte length after stuffing.
 *         3. offsets: one workgroup, an exclusive int64 scan over intervals and frames in index order (no atomics), adding the
 *            header per frame and 2 bytes per RSTm / EOI: each interval's offset and offsets[0 .. N].
 *   write 4. one workgroup per interval packs the windows again, stuffs, and stores the bytes at their final offset (dword stores
 *            between the unaligned ends), then its RSTm or EOI; the workgroup of a frame's first interval writes the header.
 * No buffer is sized by a block's worst case.  workspace: tcj_mjpeg_workspace's byte count, aligned to 8: 128 bytes of coefficients
 * and 4 of bit offset per block, 16 per interval.  Same input, same bytes; no floating point anywhere.
 *
 * The checks, in this order.  TC_ERR_ARG: a NULL pointer; N < 1; W or H < 1; quality outside 1 .. 100; a subsampling that is neither
 * constant; a negative stride.  TC_ERR_UNSUPPORTED: W or H above TC_MJPEG_MAX_SIDE; more than 2^31 - 1 blocks or 2^31 - 1 intervals.
 * TC_ERR_ARG: workspace_bytes below tcj_mjpeg_workspace's; data_bytes < 0.  TC_ERR_ALIGN: workspace not aligned to 8 bytes.
 * tcj_mjpeg_write takes the arguments tcj_mjpeg_plan was given and the workspace it filled; an interval that would end beyond
 * data_bytes is not written (offsets[N] bytes are needed). */
#ifndef TCDIFF_MJPEG_H
#define TCDIFF_MJPEG_H

#include "tcdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TC_MJPEG_444 0
#define TC_MJPEG_420 1
#define TC_MJPEG_THREADS 256
#define TC_MJPEG_WINDOW 8192
#define TC_MJPEG_LAUNCHES 4
#define TC_MJPEG_HEADER_BYTES 625
#define TC_MJPEG_MAX_SIDE 65535
#define TC_MJPEG_DCT_BITS 14
#define TC_MJPEG_COEF_BITS 20
#define TC_MJPEG_DCT_BOUND_MILLI 200

/* bytes[0] (a HOST long) = the workspace tcj_mjpeg_plan and tcj_mjpeg_write need for N frames of H x W */
int tcj_mjpeg_workspace(int N, int H, int W, int subsampling, long* bytes);

/* launches 1 - 3: fills workspace and offsets [N + 1] int64 (offsets[n] = the first byte of frame n, offsets[N] = the total) */
int tcj_mjpeg_plan(const unsigned char* frames, const long* strides, int N, int H, int W, int quality, int subsampling,
                   void* workspace, long workspace_bytes, long* offsets, hipStream_t stream);

/* launch 4: data [data_bytes] uint8, data_bytes >= offsets[N] */
int tcj_mjpeg_write(int N, int H, int W, int quality, int subsampling, const void* workspace, long workspace_bytes,
                    unsigned char* data, long data_bytes, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TCDIFF_MJPEG_H */
