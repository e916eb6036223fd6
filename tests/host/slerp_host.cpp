// Host build (g++) of quat_slerp from tcdiff_amd/csrc/fk_math.h, the slerp the pose export kernel (csrc/export.hip) runs,
// exported for tests/test_render_export_cpu.py (compared there with a float64 slerp).
#include "fk_math.h"

extern "C" {
// x, y: [n][4] real-first quaternions, a: [n] weights -> out [n][4]
void host_quat_slerp(const float* x, const float* y, const float* a, long n, float* out) {
    for (long i = 0; i < n; ++i) {
        const Q4 r = quat_slerp(q4(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]),
                                q4(y[4 * i], y[4 * i + 1], y[4 * i + 2], y[4 * i + 3]), a[i]);
        out[4 * i] = r.w; out[4 * i + 1] = r.x; out[4 * i + 2] = r.y; out[4 * i + 3] = r.z;
    }
}
}
