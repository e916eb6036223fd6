// csrc/mjpeg_math.h built for the host: the arithmetic of the HIP kernels of csrc/mjpeg.hip as a stand-alone program, run by
// tests/test_mjpeg_cpu.py under the address and undefined-behaviour sanitizers.
//   mjpeg_host in.bin out.bin
// in.bin: int32 N, H, W, quality, subsampling, then the frames [N][H][W][3] uint8.  out.bin: int64 offsets [N + 1], then the streams.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mjpeg_math.h"

struct bit_writer {
    std::vector<unsigned char> bytes;
    unsigned long long acc = 0;
    int n = 0;
    void operator()(unsigned code, int len) {
        acc = acc << len | code, n += len;
        while (n >= 8) bytes.push_back((unsigned char)(acc >> (n - 8))), n -= 8;
    }
};

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[5];
    if (fread(head, 4, 5, f) != 5) return 2;
    const int N = head[0], H = head[1], W = head[2], quality = head[3], sub = head[4];
    std::vector<unsigned char> frames((size_t)N * H * W * 3);
    if (fread(frames.data(), 1, frames.size(), f) != frames.size()) return 2;
    fclose(f);
    unsigned char qt[2][64];
    tcj_quant_tables(quality, qt);
    tcj_header hd;
    tcj_make_header(&hd, W, H, sub, qt);
    const int side = tcj_mcu_side(sub), R = (H + side - 1) / side, M = (W + side - 1) / side, bpm = tcj_mcu_blocks(sub), nb = M * bpm;
    std::vector<unsigned char> out;
    std::vector<int64_t> offsets;
    std::vector<short> coef((size_t)nb * 64);
    for (int n = 0; n < N; ++n) {
        offsets.push_back((int64_t)out.size());
        out.insert(out.end(), hd.b, hd.b + TC_MJPEG_HEADER_BYTES);
        const unsigned char* frame = frames.data() + (size_t)n * H * W * 3;
        for (int row = 0; row < R; ++row) {
            int bits = 0;
            for (int j = 0; j < nb; ++j) {
                const int m = j / bpm, k = j % bpm, chroma = tcj_block_component(sub, k) != 0;
                int s[64], t[64];
                for (int i = 0; i < 64; ++i) s[i] = tcj_sample(frame, 3L * W, 3, H, W, sub, row, m, k, i >> 3, i & 7);
                for (int i = 0; i < 64; ++i) t[i] = tcj_dct_pass1(&s[(i >> 3) * 8], i & 7);
                int run = 0;
                short* zz = &coef[(size_t)j * 64];
                for (int i = 0; i < 64; ++i) {
                    int q = tcj_quantise(tcj_dct_pass2(&t[i & 7], 8, i >> 3), qt[chroma][i]);
                    if (i) q = tcj_clamp(q, 1023);
                    zz[TCJ_UNZIGZAG.v[i]] = (short)q;
                }
                for (int i = 1; i < 64; ++i) {                 // the kernel's bit count, checked against what is written below
                    if (zz[i] == 0) {
                        ++run;
                        continue;
                    }
                    bits += tcj_ac_bits(chroma, run, zz[i]), run = 0;
                }
                if (run) bits += (int)(TCJ_AC_CODES[chroma].v[0] >> 16);
            }
            bit_writer put;
            for (int j = 0; j < nb; ++j) {
                const int pj = tcj_pred_block(sub, j), chroma = tcj_block_component(sub, j % bpm) != 0;
                const int d = tcj_dc_difference(coef[(size_t)j * 64], pj < 0 ? 0 : coef[(size_t)pj * 64]);
                bits += tcj_dc_bits(chroma, d);
                tcj_block_symbols(&coef[(size_t)j * 64], d, chroma, put);
            }
            if ((int)put.bytes.size() * 8 + put.n != bits) return 3;
            if (put.n) put((1u << (8 - put.n)) - 1, 8 - put.n);
            for (unsigned char c : put.bytes) {
                out.push_back(c);
                if (c == 0xFF) out.push_back(0);
            }
            out.push_back(0xFF);
            out.push_back((unsigned char)(row + 1 < R ? 0xD0 + (row & 7) : 0xD9));
        }
    }
    offsets.push_back((int64_t)out.size());
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(offsets.data(), 8, offsets.size(), f);
    fwrite(out.data(), 1, out.size(), f);
    fclose(f);
    return 0;
}
