// usip_amd/csrc/unit_columns_cpu.cpp -- host twin of csrc/unit_columns.hip: the same arithmetic
// (csrc/unit_math.h) on host pointers, in the device's order -- a column's channels ascending, once for the float64 sum and
// once for the outputs.  Threads split the positions (b, m), nothing else: no sum crosses a position.  Never reached from the
// device entry points.
#include "unit_math.h"
#include "host_split.h"
#include "../../include/usip_hip.h"

using namespace usip_unit;

extern "C" int usip_unit_columns_f32_cpu(const float* x, int B, int C, int M, float eps, float* out, float* norm,
                                         int num_threads)
{
    if (bad_dims(B, C, M, eps) || !x || !out || !norm) return USIP_EINVAL;
    usip_host::split((long long)B * M, num_threads, [=](long long lo, long long hi) {
        for (long long r = lo; r < hi; ++r) {
            const long long b = r / M, m = r % M, base = b * C * M + m;
            double s = 0.0;
            for (int c = 0; c < C; ++c) s = add_square(s, x[base + (long long)c * M]);
            const float n = norm_of(s), t = divisor(n, eps);
            norm[r] = n;
            for (int c = 0; c < C; ++c) out[base + (long long)c * M] = scaled(x[base + (long long)c * M], t);
        }
    });
    return USIP_OK;
}

extern "C" int usip_unit_columns_backward_f32_cpu(const float* grad, const float* x, const float* norm, int B, int C, int M,
                                                  float eps, float* dx, int num_threads)
{
    if (bad_dims(B, C, M, eps) || !grad || !x || !norm || !dx) return USIP_EINVAL;
    usip_host::split((long long)B * M, num_threads, [=](long long lo, long long hi) {
        for (long long r = lo; r < hi; ++r) {
            const long long b = r / M, m = r % M, base = b * C * M + m;
            double dot = 0.0;
            for (int c = 0; c < C; ++c) dot = add_product(dot, grad[base + (long long)c * M], x[base + (long long)c * M]);
            const float n = norm[r], t = divisor(n, eps);
            for (int c = 0; c < C; ++c)
                dx[base + (long long)c * M] = grad_of(grad[base + (long long)c * M], x[base + (long long)c * M], dot, n, t);
        }
    });
    return USIP_OK;
}
