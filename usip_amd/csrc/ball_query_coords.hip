// usip_amd/csrc/ball_query_coords.hip -- fused coords-in ball query on gfx950.
//
// Same result, bit for bit, as usip_pairwise_dist_f32 followed by usip_ball_query_f32
// (models/networks.py:694-698 + ball_query_cuda.cu:22-46) without the B x M x N matrix ever
// touching HBM: a wave owns R node rows of one cloud, streams the cloud's coordinates (L2
// resident, 12 B per point) once for all R rows and evaluates the distance test in registers.
//
// Bit-exactness of the fused test: the reference compares sqrt_rn(s) <= radius with
// s = fma(dz,dz,fma(dy,dy,dx*dx)).  sqrt_rn is monotone, so there is a largest float T with
// sqrt_rn(T) <= radius and the test is exactly  s <= T.  T is found once per call by probing
// the neighbours of radius^2 with a correctly rounded sqrt (usip_sqrt_threshold, pair_scan.h, on the host).
#include "pair_scan.h"
#include <cstdlib>

namespace {

// R = node rows per wave: every point a wave loads is tested against R nodes (fewer L2 bytes per test), but a launch has
// only B * M / R waves -- 2048 at R = 4 for the detector's 16 clouds of 512 nodes, two per SIMD, too few to hide the L2
// round trip of the next block of points behind the tests of the current one.
template <bool VEC, int R>
__global__ __launch_bounds__(256) void ball_query_coords_kernel(
    const float* __restrict__ node, const float* __restrict__ x, int32_t* __restrict__ out,
    float T, int K, int M, int N)
{
    extern __shared__ __attribute__((aligned(16))) int smem[];      // [4 waves][R][K]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int m0 = (blockIdx.x * 4 + wave) * R;
    int* lists = smem + wave * R * K;
    const float* xb = x + (long long)b * 3 * N;
    const float* nb = node + (long long)b * 3 * M;

    int count[R];
    usip_ball_scan_rows<VEC, R>(nb, xb, lists, count, T, K, M, N, m0, lane);      // pair_scan.h
    __syncthreads();
    usip_ball_write_rows<R>(lists, count, out + ((long long)b * M + m0) * K, K, M, m0, lane);
}

}  // namespace

extern "C" int usip_ball_query_coords_f32(const float* node, const float* x, int32_t* out_idx,
                                          float radius, int K, int B, int M, int N, void* stream)
{
    if (B < 0 || M < 0 || N < 0 || K < 0) return USIP_EINVAL;
    if ((long long)B * M == 0 || K == 0) return USIP_OK;
    if (!node || !x || !out_idx) return USIP_EINVAL;
    if (K > 1024 || B > 65535) return USIP_EINVAL;           // LDS: 4*R*K*4 B = 64 KiB at K=1024
    const float T = usip_sqrt_threshold(radius);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (N >= 4) && (N % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15u) == 0);
    static const int forced = [] { const char* e = getenv("USIP_BQ_ROWS"); return e ? atoi(e) : 0; }();
    // rows per wave: 4 when that still gives every SIMD four waves (>= 4096 waves), else 2, else 1
    const long long rows = (long long)B * M;
    int R = rows >= 4 * 4096 ? 4 : (rows >= 2 * 4096 ? 2 : 1);
    if (forced == 1 || forced == 2 || forced == 4) R = forced;
    dim3 grid(usip_ceil_div(M, 4 * R), B), block(256);
    const size_t lds = (size_t)4 * R * K * sizeof(int);
#define USIP_BQC(V_, R_) USIP_LAUNCH((ball_query_coords_kernel<V_, R_>), grid, block, lds, st, node, x, out_idx, T, K, M, N)
    if (vec) { if (R == 4) USIP_BQC(true, 4); else if (R == 2) USIP_BQC(true, 2); else USIP_BQC(true, 1); }
    else     { if (R == 4) USIP_BQC(false, 4); else if (R == 2) USIP_BQC(false, 2); else USIP_BQC(false, 1); }
#undef USIP_BQC
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
