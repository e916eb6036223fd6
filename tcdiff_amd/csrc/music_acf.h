// The windowed autocorrelation of an onset envelope, shared by the tempogram (music.hip, W = 384) and the beat tracker's tempo
// estimate (beat.hip, W = 480).  Definitions: include/tcdiff_hip.h.  A workgroup of W / 2 threads holds one frame's W windowed
// samples in LDS; thread k sums lags k and W - 1 - k, each in ascending sample order (W + 1 products per thread).
#pragma once
#include "common.h"

// Sample i of frame t: padded sample t + i of env[0 .. T) padded by W / 2 on both sides with a linear ramp to 0 (numpy.pad:
// sample j of the left ramp is j * (env[0] / (W / 2)), of the right one (W / 2 - 1 - j) * (env[T - 1] / (W / 2))).
template <int W>
DEVINL float mu_ramp_sample(const float* __restrict__ env, int T, int t, int i) {
    const int j = t + i - W / 2;
    float x;
    if (j < 0) x = (float)(t + i) * (env[0] / (float)(W / 2));
    else if (j >= T) x = (float)(W / 2 - 1 - (j - T)) * (env[T - 1] / (float)(W / 2));
    else x = env[j];
    return x;
}

// a = lag tid, c = lag W - 1 - tid of s_x[W]: sum_i x[i] x[i + l] over i + l < W in ascending i
template <int W>
DEVINL void mu_acf_pair(const float* s_x, int tid, float& a, float& c) {
    const int la = tid, lb = W - 1 - tid;
    a = 0.0f;
    c = 0.0f;
    for (int i = 0; i + la < W; ++i) a += s_x[i] * s_x[i + la];
    for (int i = 0; i + lb < W; ++i) c += s_x[i] * s_x[i + lb];
}

// max_l |a[l]| over the W lags the W / 2 <= 256 threads hold; s_red[256].  Every thread returns it; the caller puts a barrier
// in front of the next use of s_red.
template <int W>
DEVINL float mu_acf_absmax(float* s_red, float a, float c, int tid) {
    static_assert(W / 2 <= 256, "the reduction tree has 256 leaves");
    s_red[tid] = fmaxf(fabsf(a), fabsf(c));
    if (tid < 256 - W / 2) s_red[W / 2 + tid] = 0.0f;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_red[tid] = fmaxf(s_red[tid], s_red[tid + o]);
        __syncthreads();
    }
    return s_red[0];
}
