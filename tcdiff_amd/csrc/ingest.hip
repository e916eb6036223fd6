// The motion side of AIOZDataset.process_dataset (reference dataset/group_dataset.py:167-238), gfx950, fp32, two launches
// for any number of clips: raw SMPL motion (root positions, 24 axis-angle rotations per pose, Y-up) -> the normalised
// 151-column rows the diffusion trains on.  The inverse of csrc/export.hip.
//
//   root rotation and position, Y-up -> Z-up        dataset/group_dataset.py:183-198
//   SMPLSkeleton.forward, foot contacts             dataset/group_dataset.py:201-207, vis.py:358-406
//   ax_to_6v                                        dataset/group_dataset.py:210, dataset/quaternion.py:21-25
//   row layout [contacts 4 | root 3 | 6-D 24 x 6]   dataset/group_dataset.py:213-214, dataset/preprocess.py:46-54
//   Normalizer fit (one per clip) and transform     dataset/group_dataset.py:217-221, dataset/scaler.py:50-78
//
// ingest_pose_kernel: one thread per pose (clip, dancer, frame); the per-pose arithmetic is csrc/fk_math.h.
// ingest_clip_kernel: one workgroup per clip -- contacts need the next frame's feet, the fit needs every row of the clip.
// One-off preprocessing, a few hundred thousand poses per dataset: no LDS tiling, no MFMA.
#include "common.h"
#include "fk_math.h"
#include "tcdiff_hip.h"

#define TC_INGEST_C 151           // 4 contacts, 3 root, 24 x 6 rotation
#define TC_INGEST_FEET 4
#define TC_INGEST_GROUPS 4        // row groups of the column reduction
#define TC_INGEST_THREADS 640     // >= TC_INGEST_GROUPS * TC_INGEST_C

__global__ __launch_bounds__(64) void ingest_pose_kernel(const float* __restrict__ pos, const float* __restrict__ q, FkSkel sk,
                                                        long P, float* __restrict__ feats, float* __restrict__ feet) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    float aa[TC_FK_J * 3], jt[TC_FK_J * 3], root[3];
#pragma unroll
    for (int k = 0; k < TC_FK_J * 3; ++k) aa[k] = q[p * (TC_FK_J * 3) + k];
    const V3 r0 = root_yup_to_zup(v3(aa[0], aa[1], aa[2]));
    aa[0] = r0.x; aa[1] = r0.y; aa[2] = r0.z;
    const V3 rp = rotate_x90(v3(pos[p * 3], pos[p * 3 + 1], pos[p * 3 + 2]));
    root[0] = rp.x; root[1] = rp.y; root[2] = rp.z;
    fk_forward(aa, root, sk, jt, nullptr);
    float* row = feats + p * TC_INGEST_C;
    for (int c = 0; c < 3; ++c) row[4 + c] = root[c];
    for (int j = 0; j < TC_FK_J; ++j) {
        float d6[6];
        rot6_from_quat(quat_from_axis_angle(v3(aa[3 * j], aa[3 * j + 1], aa[3 * j + 2])), d6);
#pragma unroll
        for (int k = 0; k < 6; ++k) row[7 + 6 * j + k] = d6[k];
    }
    const int foot[TC_INGEST_FEET] = {7, 8, 10, 11};          // dataset/group_dataset.py:204
    for (int f = 0; f < TC_INGEST_FEET; ++f)
        for (int k = 0; k < 3; ++k) feet[p * (TC_INGEST_FEET * 3) + 3 * f + k] = jt[3 * foot[f] + k];
}

// torch.min / torch.max propagate NaN
DEVINL float min_nan(float m, float v) { return (v < m || v != v) ? v : m; }
DEVINL float max_nan(float m, float v) { return (v > m || v != v) ? v : m; }

__global__ __launch_bounds__(TC_INGEST_THREADS) void ingest_clip_kernel(const float* __restrict__ feet, int dn, int sq, int fit,
                                                                       const float* __restrict__ scale_in,
                                                                       const float* __restrict__ min_in, float* feats,
                                                                       float* __restrict__ raw, float* __restrict__ stats) {
#pragma clang fp contract(off)      // difference, norm, scale_ / min_ and the transform round after every operation
    __shared__ float s_lo[TC_INGEST_GROUPS][TC_INGEST_C], s_hi[TC_INGEST_GROUPS][TC_INGEST_C];
    __shared__ float s_scale[TC_INGEST_C], s_min[TC_INGEST_C];
    const int clip = blockIdx.x, tid = threadIdx.x;
    const long R = (long)dn * sq;                       // rows of this clip
    float* x = feats + (long)clip * R * TC_INGEST_C;
    const float* ft = feet + (long)clip * R * (TC_INGEST_FEET * 3);
    // contacts: |feet[t + 1] - feet[t]| < 0.01 within one dancer; the last frame's speed is 0, so its contact is 1
    for (long i = tid; i < R * TC_INGEST_FEET; i += TC_INGEST_THREADS) {
        const long r = i / TC_INGEST_FEET;
        const int f = (int)(i - r * TC_INGEST_FEET);
        const int t = (int)(r % sq);
        float v = 0.0f;
        if (t < sq - 1) {
            const float* a = ft + r * (TC_INGEST_FEET * 3) + 3 * f;
            const float* b = a + TC_INGEST_FEET * 3;
            const float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
            v = sqrtf(dx * dx + dy * dy + dz * dz);
        }
        x[r * TC_INGEST_C + f] = v < 0.01f ? 1.0f : 0.0f;
    }
    __syncthreads();
    if (fit) {
        // dataset/scaler.py:58-70 over this clip's rows; min and max do not depend on the order
        const int g = tid / TC_INGEST_C, c = tid - g * TC_INGEST_C;
        if (g < TC_INGEST_GROUPS) {
            float lo = x[c], hi = lo;                   // row 0: every group starts from a value of the column
            for (long r = g; r < R; r += TC_INGEST_GROUPS) {
                const float v = x[r * TC_INGEST_C + c];
                lo = min_nan(lo, v);
                hi = max_nan(hi, v);
            }
            s_lo[g][c] = lo;
            s_hi[g][c] = hi;
        }
        __syncthreads();
        if (tid < TC_INGEST_C) {
            float lo = s_lo[0][tid], hi = s_hi[0][tid];
            for (int k = 1; k < TC_INGEST_GROUPS; ++k) {
                lo = min_nan(lo, s_lo[k][tid]);
                hi = max_nan(hi, s_hi[k][tid]);
            }
            float range = hi - lo;
            if (range < 10.0f * 1.1920929e-07f) range = 1.0f;          // _handle_zeros_in_scale
            const float sc = 2.0f / range;
            const float mn = -1.0f - lo * sc;
            float* st = stats + (long)clip * 4 * TC_INGEST_C;
            st[tid] = lo;
            st[TC_INGEST_C + tid] = hi;
            st[2 * TC_INGEST_C + tid] = sc;
            st[3 * TC_INGEST_C + tid] = mn;
            s_scale[tid] = sc;
            s_min[tid] = mn;
        }
    } else if (tid < TC_INGEST_C) {
        s_scale[tid] = scale_in[tid];
        s_min[tid] = min_in[tid];
    }
    __syncthreads();
    float* rw = raw ? raw + (long)clip * R * TC_INGEST_C : nullptr;
    for (long i = tid; i < R * TC_INGEST_C; i += TC_INGEST_THREADS) {
        const int c = (int)(i % TC_INGEST_C);
        const float v = x[i];
        if (rw) rw[i] = v;
        float y = v * s_scale[c];
        y = y + s_min[c];
        x[i] = y < -1.0f ? -1.0f : (y > 1.0f ? 1.0f : y);          // torch.clip keeps NaN
    }
}

extern "C" int tcdiff_motion_ingest(const float* pos, const float* q, int clips, int dn, int sq, const int* parents,
                                    const float* offsets, int fit, const float* scale, const float* min_, float* feats,
                                    float* raw, float* feet, float* stats, hipStream_t stream) {
    if (!pos || !q || !parents || !offsets || !feats || !feet) return TC_ERR_ARG;
    if (clips < 1 || dn < 1 || sq < 1) return TC_ERR_ARG;
    if (fit ? !stats : (!scale || !min_)) return TC_ERR_ARG;
    FkSkel sk;
    for (int j = 0; j < TC_FK_J; ++j) sk.has_children[j] = 0;
    for (int j = 0; j < TC_FK_J; ++j) {
        sk.parent[j] = parents[j];
        if (parents[j] >= j) return TC_ERR_ARG;          // a parent must precede its children
        if (parents[j] >= 0) sk.has_children[parents[j]] = 1;
        for (int k = 0; k < 3; ++k) sk.off[j][k] = offsets[3 * j + k];
    }
    const long P = (long)clips * dn * sq;
    if ((P + 63) / 64 > 0x7fffffffL) return TC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(ingest_pose_kernel, dim3((unsigned)((P + 63) / 64)), dim3(64), 0, stream, pos, q, sk, P, feats, feet);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(ingest_clip_kernel, dim3((unsigned)clips), dim3(TC_INGEST_THREADS), 0, stream, feet, dn, sq, fit ? 1 : 0,
                       scale, min_, feats, raw, stats);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
