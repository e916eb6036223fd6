// Host build (g++) of the motion-ingest functions of tcdiff_amd/csrc/fk_math.h (the source csrc/ingest.hip runs per pose),
// exported for tests/test_ingest_cpu.py (compared there with the float64 restatement tests/ingest_ref.py).
#include "fk_math.h"

extern "C" {
// q: [n][4] real-first quaternions (any length) -> out [n][6], the first two rows of the rotation matrix
void host_rot6_from_quat(const float* q, long n, float* out) {
    for (long i = 0; i < n; ++i) rot6_from_quat(q4(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]), out + 6 * i);
}
// aa: [n][3] axis-angle -> out [n][6] = ax_to_6v(aa) as the ingest kernel evaluates it
void host_ax_to_6v(const float* aa, long n, float* out) {
    for (long i = 0; i < n; ++i)
        rot6_from_quat(quat_from_axis_angle(v3(aa[3 * i], aa[3 * i + 1], aa[3 * i + 2])), out + 6 * i);
}
// aa: [n][3] Y-up root axis-angle -> out [n][3] Z-up
void host_root_yup_to_zup(const float* aa, long n, float* out) {
    for (long i = 0; i < n; ++i) {
        const V3 r = root_yup_to_zup(v3(aa[3 * i], aa[3 * i + 1], aa[3 * i + 2]));
        out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
    }
}
// p: [n][3] Y-up positions -> out [n][3] Z-up
void host_rotate_x90(const float* p, long n, float* out) {
    for (long i = 0; i < n; ++i) {
        const V3 r = rotate_x90(v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]));
        out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
    }
}
}
