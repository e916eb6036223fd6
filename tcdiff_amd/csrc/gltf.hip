// The binary block of an animated glTF file, gfx950: exported SMPL poses -> key-frame times, root translations turned to Y-up and
// per-joint quaternions whose sign is continuous in time.  float64 arithmetic on the float32 inputs, contraction off
// (csrc/gltf_math.h holds the quaternion and the flip test, and compiles for the host too), no atomics, no workspace: the same
// input gives the same bits.  The definitions: include/tcdiff_gltf.h.
//
//   gltf_animation_kernel   a wave per channel, four waves per workgroup: per (clip, dancer) 24 rotation channels and a 25th wave
//                           that copies trans (and, for dancer 0, writes times).  A rotation wave walks its channel 64 frames per
//                           pass, lane = frame: the lane builds q_t and, from the previous frame's rotation vector, q_(t-1) again
//                           (the same bits, cheaper than four float64 shuffles), the wave ballots "the sign flips here", and a
//                           lane's sign is the parity of the flips at or before it, XORed with the wave-uniform carry of the
//                           passes before.  A lane stores its 16 bytes next to its neighbours'; a channel need not start on a
//                           16-byte boundary (T, dn and the caller's pointer decide), so the store is declared 4-byte aligned.
#include "common.h"
#include "gltf_math.h"
#include "tcdiff_gltf.h"

#define TC_GLTF_THREADS 256
#define TC_GLTF_WAVES (TC_GLTF_THREADS / TC_WAVE)
#define TC_GLTF_CHANNELS (TC_GLTF_JOINTS + 1)             // waves per (clip, dancer)

static_assert(TC_GLTF_FLOATS(1, 1) == 1 + TC_GLTF_PER_DANCER && TC_GLTF_PER_DANCER == 3 + 4 * TC_GLTF_JOINTS,
              "gltf_math.h and the header disagree");

struct __attribute__((packed, aligned(4))) GltfStore { float x, y, z, w; };

__global__ __launch_bounds__(TC_GLTF_THREADS) void gltf_animation_kernel(const float* __restrict__ poses,
                                                                        const float* __restrict__ trans, long waves, int T, int dn,
                                                                        double fps, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x % TC_WAVE;
    const long w = (long)blockIdx.x * TC_GLTF_WAVES + threadIdx.x / TC_WAVE;
    if (w >= waves) return;                               // wave-uniform
    const long cd = w / TC_GLTF_CHANNELS;                 // clip * dn + dancer
    const int ch = (int)(w - cd * TC_GLTF_CHANNELS);
    const long c = cd / dn;
    const int d = (int)(cd - c * dn);
    float* clip = out + c * TC_GLTF_FLOATS(T, dn);
    float* dancer = clip + T + (long)d * TC_GLTF_PER_DANCER * T;
    if (ch == TC_GLTF_JOINTS) {                           // the 25th wave: trans, and times once per clip
        for (int t = lane; t < T; t += TC_WAVE) {
            const float* p = trans + ((c * T + t) * dn + d) * 3;
            float* o = dancer + 3L * t;
            o[0] = p[0];
            o[1] = p[2];
            o[2] = -p[1];
            if (d == 0) clip[t] = (float)((double)t / fps);
        }
        return;
    }
    const float* R = poses + ((c * T) * dn + d) * 72 + 3 * ch;          // frame t at R + t * dn * 72
    const long fs = 72L * dn;
    GltfStore* o = reinterpret_cast<GltfStore*>(dancer + 3L * T + 4L * ch * T);
    const unsigned long long upto = (2ULL << lane) - 1ULL;             // lanes <= this one (lane 63: all)
    int carry = 0;                                                      // parity of the flips of the passes before
    for (int t0 = 0; t0 < T; t0 += TC_WAVE) {
        const int t = t0 + lane;
        GltfQ q = {0.0, 0.0, 0.0, 1.0};
        int flip = 0;
        if (t < T) {
            q = gltf_quat(R + t * fs, ch == 0);
            flip = t == 0 ? q.w < 0.0 : gltf_flips(gltf_quat(R + (t - 1) * fs, ch == 0), q);
        }
        const unsigned long long m = __ballot(flip);
        const double s = ((__popcll(m & upto) ^ carry) & 1) ? -1.0 : 1.0;
        carry ^= __popcll(m) & 1;
        if (t < T) {
            GltfStore v;
            v.x = (float)(s * q.x);
            v.y = (float)(s * q.y);
            v.z = (float)(s * q.z);
            v.w = (float)(s * q.w);
            o[t] = v;
        }
    }
}

extern "C" int tcx_gltf_animation(const float* smpl_poses, const float* smpl_trans, int clips, int T, int dn, double fps,
                                  float* out, hipStream_t stream) {
    if (!smpl_poses || !smpl_trans || !out) return TC_ERR_ARG;
    if (clips < 1 || T < 1 || dn < 1) return TC_ERR_ARG;
    if (!(fps > 0.0) || !(fps <= 1.7976931348623157e308)) return TC_ERR_ARG;
    const long lim = 0x7fffffffL;
    const long per = 1L + TC_GLTF_PER_DANCER * (long)dn;               // F = T * per exceeds both inputs' elements per clip
    if (per > lim / T || per * T > lim / clips) return TC_ERR_UNSUPPORTED;
    const long waves = (long)clips * dn * TC_GLTF_CHANNELS;            // < clips * F
    hipLaunchKernelGGL(gltf_animation_kernel, dim3((unsigned)((waves + TC_GLTF_WAVES - 1) / TC_GLTF_WAVES)), dim3(TC_GLTF_THREADS),
                       0, stream, smpl_poses, smpl_trans, waves, T, dn, fps, out);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
