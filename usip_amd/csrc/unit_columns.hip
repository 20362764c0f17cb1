// usip_amd/csrc/unit_columns.hip -- out = x / (|x| + eps) over the channels of x f32 [B][C][M], and its backward, on the device
// (the last line of the reference's DescriptorLiteOldGlobal, models/networks.py:477).  csrc/unit_math.h has the
// arithmetic, which the host twin (csrc/unit_columns_cpu.cpp) shares.  One launch each way instead of three ATen launches
// forward (norm, add, divide) and about six backward.
//
//   unit_columns_kernel           one lane per position (b, m), 64 lanes per workgroup, a grid-stride loop beyond MAX_GRID
//   unit_columns_backward_kernel  workgroups.  The lane walks its column's C channels in ascending order, twice: once for the
//                                 float64 sum, once for the outputs.  Lane l and lane l + 1 hold neighbouring m, so every
//                                 load and store of a wave is one run of consecutive addresses (a run that crosses into the
//                                 next batch element where m wraps).  No LDS, no cross-lane step, no atomics: the order of
//                                 every sum is the channel order, whatever the launch geometry.
// The second walk re-reads what the first one read; a column set of B * C * M * 4 bytes (1 MB at the indoor shape) stays in L2.
#include "common.h"
#include "unit_math.h"

using namespace usip_unit;

namespace {

constexpr int TILE = 64;
constexpr long long MAX_GRID = 1LL << 16;        // workgroups of a launch (4 M positions a sweep); the kernels loop beyond it

__global__ __launch_bounds__(TILE) void unit_columns_kernel(const float* __restrict__ x, long long rows, int C, int M, float eps,
                                                            float* __restrict__ out, float* __restrict__ norm)
{
    const long long stride = (long long)gridDim.x * TILE;
    for (long long r = (long long)blockIdx.x * TILE + threadIdx.x; r < rows; r += stride) {
        const long long b = r / M, m = r % M, base = b * C * M + m;
        double s = 0.0;
#pragma unroll 4
        for (int c = 0; c < C; ++c) s = add_square(s, x[base + (long long)c * M]);
        const float n = norm_of(s), t = divisor(n, eps);
        norm[r] = n;
#pragma unroll 4
        for (int c = 0; c < C; ++c) out[base + (long long)c * M] = scaled(x[base + (long long)c * M], t);
    }
}

__global__ __launch_bounds__(TILE) void unit_columns_backward_kernel(const float* __restrict__ grad,
                                                                     const float* __restrict__ x,
                                                                     const float* __restrict__ norm, long long rows, int C,
                                                                     int M, float eps, float* __restrict__ dx)
{
    const long long stride = (long long)gridDim.x * TILE;
    for (long long r = (long long)blockIdx.x * TILE + threadIdx.x; r < rows; r += stride) {
        const long long b = r / M, m = r % M, base = b * C * M + m;
        double dot = 0.0;
#pragma unroll 4
        for (int c = 0; c < C; ++c) dot = add_product(dot, grad[base + (long long)c * M], x[base + (long long)c * M]);
        const float n = norm[r], t = divisor(n, eps);
#pragma unroll 4
        for (int c = 0; c < C; ++c)
            dx[base + (long long)c * M] = grad_of(grad[base + (long long)c * M], x[base + (long long)c * M], dot, n, t);
    }
}

dim3 grid_for(long long rows)
{
    const long long blocks = (rows + TILE - 1) / TILE;
    return dim3((unsigned)(blocks < MAX_GRID ? blocks : MAX_GRID));
}

}  // namespace

extern "C" int usip_unit_columns_f32(const float* x, int B, int C, int M, float eps, float* out, float* norm, void* stream)
{
    if (bad_dims(B, C, M, eps) || !x || !out || !norm) return USIP_EINVAL;
    const long long rows = (long long)B * M;
    if (rows == 0) return USIP_OK;
    USIP_LAUNCH(unit_columns_kernel, grid_for(rows), dim3(TILE), 0, (hipStream_t)stream, x, rows, C, M, eps, out, norm);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_unit_columns_backward_f32(const float* grad, const float* x, const float* norm, int B, int C, int M,
                                              float eps, float* dx, void* stream)
{
    if (bad_dims(B, C, M, eps) || !grad || !x || !norm || !dx) return USIP_EINVAL;
    const long long rows = (long long)B * M;
    if (rows == 0) return USIP_OK;
    USIP_LAUNCH(unit_columns_backward_kernel, grid_for(rows), dim3(TILE), 0, (hipStream_t)stream, grad, x, norm, rows, C, M, eps,
                dx);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
