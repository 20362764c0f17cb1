// usip_amd/csrc/loss_tail.hip -- the detector step's loss segment, keypoints / sigmas to their gradients, as three
// launches (gfx950).
//
// Between the detector head and its backward the step ran a chain of small dependent launches over 2 x M keypoints per
// pair (models/keypoint_detector.py:182-204): the rigid transform (head.hip), two nearest-keypoint scans and their four
// backward kernels (nearest.hip), the sigma arithmetic each way (chamfer.hip), the loss combination and the fill of
// its gradient (head.hip), the backward of the keypoint-on-cloud distance, and what autograd adds around them (the
// backward of torch.split, two gradient sums).  Every one is a few microseconds of a 64-256 workgroup launch inside
// the captured step, and all the operands of one pair fit in one workgroup's LDS.  Here:
//   loss_tail_scan_kernel   t = (R scale) p + shift for the pair, then both directions of the keypoint scan on LDS copies
//   loss_tail_sums_kernel   the chamfer sums, the two on-cloud means, the six scalars of the step's loss
//   loss_tail_bwd_kernel    from dL/dloss to dL/dkeypoints and dL/dsigmas in one launch
// The arithmetic is the chain's own, operation for operation: the scan is usip_nearest_scan (pair_scan.h), the sums are
// block_sum4 / side_sums / Side (chamfer_sums.h), and the lines taken from head.hip and nearest.hip name their source.
// The keypoint-on-cloud search between the first two stays its own launch (cell_grid.hip or nearest.hip).
#include "chamfer_sums.h"
#include "pair_scan.h"

namespace {

constexpr int ROWS = 4;              // query points per wave, as nearest_kernel (its R)
constexpr int TAIL_MAX_M = 1024;     // one staging chunk: CHUNK of chamfer.hip, BWD_CHUNK of nearest.hip

// Grid (ceil(M / 16), B): a workgroup forms every t_i of its pair (rigid_kernel<false>'s arithmetic: a = R * scale
// rounded first, then one product and two fused multiply-adds, then shift + t), stages q beside it and answers 16 rows
// of both directions with nearest_kernel's scan over the whole candidate range.
__global__ __launch_bounds__(256) void loss_tail_scan_kernel(
    const float* __restrict__ kp, const float* __restrict__ Rm, const float* __restrict__ scale,
    const float* __restrict__ shift, float* __restrict__ kp_t, float* __restrict__ a, int32_t* __restrict__ J,
    float* __restrict__ c, int32_t* __restrict__ I, int B, int M)
{
    __shared__ float s_t[3 * TAIL_MAX_M];
    __shared__ float s_q[3 * TAIL_MAX_M];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    const float* xb = kp + (long long)b * 3 * M;
    const float* qb = kp + (long long)(B + b) * 3 * M;
    const float s = scale[b];
    const float* r = Rm + b * 9;
    for (int m = threadIdx.x; m < M; m += 256) {
        const float x0 = xb[m], x1 = xb[M + m], x2 = xb[2 * M + m];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float a0 = r[3 * i] * s, a1 = r[3 * i + 1] * s, a2 = r[3 * i + 2] * s;
            float t = a0 * x0;
            t = __builtin_fmaf(a1, x1, t);
            t = __builtin_fmaf(a2, x2, t);
            s_t[i * M + m] = shift[b * 3 + i] + t;
            s_q[i * M + m] = qb[i * M + m];
        }
    }
    __syncthreads();
    const int m0 = blockIdx.x * 4 * ROWS;
    if (threadIdx.x < 3 * 4 * ROWS) {                            // this workgroup's rows of kp_t
        const int i = threadIdx.x / (4 * ROWS), m = m0 + threadIdx.x % (4 * ROWS);
        if (m < M) kp_t[((long long)b * 3 + i) * M + m] = s_t[i * M + m];
    }
    const int i0 = m0 + wave * ROWS;
    if (i0 >= M) return;
    float d[ROWS];
    int j[ROWS];
    usip_nearest_scan<ROWS>(s_t, s_q, M, M, 0, M, i0, lane, d, j);                  // pair_scan.h
#pragma unroll
    for (int rr = 0; rr < ROWS; ++rr) {
        if (lane == 0 && i0 + rr < M) {
            if (j[rr] == 0x7fffffff) j[rr] = 0;                  // all-NaN row
            a[(long long)b * M + i0 + rr] = d[rr];
            J[(long long)b * M + i0 + rr] = j[rr];
        }
    }
    usip_nearest_scan<ROWS>(s_q, s_t, M, M, 0, M, i0, lane, d, j);
#pragma unroll
    for (int rr = 0; rr < ROWS; ++rr) {
        if (lane == 0 && i0 + rr < M) {
            if (j[rr] == 0x7fffffff) j[rr] = 0;
            c[(long long)b * M + i0 + rr] = d[rr];
            I[(long long)b * M + i0 + rr] = j[rr];
        }
    }
}

// One workgroup of 1024 threads: chamfer_prob_fwd_kernel's sums and roundings, then loss_combine_kernel's (head.hip)
// on d [2B][M], the keypoint-on-cloud distances with the src rows first.
// out6 = (loss, loss_chamfer, chamfer_pure, chamfer_weighted, alpha * mean(d_src), alpha * mean(d_dst))
__global__ __launch_bounds__(1024) void loss_tail_sums_kernel(
    const float* __restrict__ a, const int* __restrict__ J, const float* __restrict__ c, const int* __restrict__ I,
    const float* __restrict__ sg, const float* __restrict__ d, float alpha, float* __restrict__ out6, int B, int M)
{
    __shared__ double red[64];
    __shared__ double red2[2][16];
    const long long half = (long long)B * M;
    const float* ss = sg;
    const float* sd = sg + half;
    double f[4], g[4];
    side_sums(a, J, ss, sd, B, M, M, f, red);
    side_sums(c, I, sd, ss, B, M, M, g, red);
    double s0 = 0.0, s1 = 0.0;
    for (long long e = threadIdx.x; e < half; e += 1024) { s0 += (double)d[e]; s1 += (double)d[half + e]; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { s0 += __shfl_down(s0, off); s1 += __shfl_down(s1, off); }
    if ((threadIdx.x & 63) == 0) { red2[0][threadIdx.x >> 6] = s0; red2[1][threadIdx.x >> 6] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double nf = (double)B * M, nb = (double)B * M;
        const float chamfer = (float)(f[0] / nf) + (float)(g[0] / nb);   // forward_loss + backward_loss
        out6[1] = chamfer;
        out6[2] = (float)(f[1] / nf) + (float)(g[1] / nb);               // chamfer_pure
        out6[3] = (float)(f[3] / f[2]) + (float)(g[3] / g[2]);           // mean(w a) = sum(a/s) / sum(1/s)
        double t0 = 0.0, t1 = 0.0;
        for (int w = 0; w < 16; ++w) { t0 += red2[0][w]; t1 += red2[1][w]; }
        const double m0 = t0 / (double)half * (double)alpha, m1 = t1 / (double)half * (double)alpha;
        out6[4] = (float)m0;
        out6[5] = (float)m1;
        out6[0] = (float)((double)chamfer + (m0 + m1));
    }
}

// Grid (ceil(M / 64), B), 256 threads, as chamfer_prob_bwd_kernel: a workgroup owns 64 targets t of one pair.  Two
// passes.  Pass 0 stages, for every src keypoint i of the pair, J_i, the sigma half h_f[i] (Side::half), da_i and
// ga1_i = (t_i - q_J) * (da_i / a_i) (nearest_bwd_kernel's line); its four waves each sum a quarter of the sources that
// name target t, for the sigma and the three coordinates alike (the quarter chains of chamfer_prob_bwd_kernel and
// nearest_bwd_partner_kernel), which gives d sigma_dst[t] and gb1_t.  Pass 1 is the other direction: d sigma_src[t],
// gb2_t.  Then, per target: g_t = ga1 + gb2 and g_q = gb1 + ga2 (autograd's one addition each), g_p = (R scale)^T g_t
// (rigid_kernel<true>), the keypoint-on-cloud gradient of both rows (fill_scaled's product, nearest_bwd_kernel's line),
// and the one addition autograd makes of the two.  Every output element is written by exactly one thread.
__global__ __launch_bounds__(256) void loss_tail_bwd_kernel(
    const float* __restrict__ gloss, const float* __restrict__ kp, const float* __restrict__ sg,
    const float* __restrict__ kp_t, const float* __restrict__ a, const int* __restrict__ J,
    const float* __restrict__ c, const int* __restrict__ I, const float* __restrict__ d_on,
    const int* __restrict__ arg_on, const float* __restrict__ pc, const float* __restrict__ Rm,
    const float* __restrict__ scale, float factor, float* __restrict__ g_kp, float* __restrict__ g_sg,
    int B, int M, int N)
{
    __shared__ __attribute__((aligned(16))) int s_arg[TAIL_MAX_M];
    __shared__ __attribute__((aligned(16))) float s_val[TAIL_MAX_M];
    __shared__ __attribute__((aligned(16))) float s_g[3][TAIL_MAX_M];
    __shared__ float s_dd[TAIL_MAX_M];
    __shared__ float part[4][4][64];
    const int b = blockIdx.y, tl = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + tl;
    const float g = gloss[0];
    const long long om = (long long)b * M, on = (long long)(B + b) * M;
    const float* tp = kp_t + om * 3;                          // the transformed src keypoints of the pair
    const float* qp = kp + on * 3;                            // its dst keypoints
    const Side fwd{a + om, J + om, sg + om, sg + on, g / ((float)B * (float)M)};
    const Side bwd{c + om, I + om, sg + on, sg + om, g / ((float)B * (float)M)};
    const int len4 = ((M + 15) / 16) * 4;                     // sources per wave, a multiple of 4
    float dsig[2] = {0.f, 0.f}, ga1[3] = {0.f, 0.f, 0.f}, g_q[3] = {0.f, 0.f, 0.f}, g_t[3] = {0.f, 0.f, 0.f};
    for (int pass = 0; pass < 2; ++pass) {
        const Side& src = pass == 0 ? fwd : bwd;              // pass 0: h_f[i] and ga1_i land on dst keypoint J[i]
        const Side& own = pass == 0 ? bwd : fwd;
        const float* ap = pass == 0 ? tp : qp;
        const float* bp = pass == 0 ? qp : tp;
        __syncthreads();
        for (int i = threadIdx.x; i < 4 * len4; i += 256) {
            if (i < M) {
                s_val[i] = src.half(i, s_dd);                 // s_dd[i] = dL/dd of this direction (da or dc)
                const int k = src.arg[i];
                const float dist = src.d[i];
                const float sc = dist > 0.f ? s_dd[i] / dist : 0.f;
                s_arg[i] = k;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) s_g[ch][i] = (ap[ch * M + i] - bp[ch * M + k]) * sc;
            } else {
                s_arg[i] = -1;
                s_val[i] = 0.f;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) s_g[ch][i] = 0.f;
            }
        }
        __syncthreads();
        float acc = 0.f, ac0 = 0.f, ac1 = 0.f, ac2 = 0.f;
        for (int i = q * len4; i < (q + 1) * len4; i += 4) {
            const int4 k = *reinterpret_cast<const int4*>(&s_arg[i]);
            const float4 v = *reinterpret_cast<const float4*>(&s_val[i]);
            const float4 v0 = *reinterpret_cast<const float4*>(&s_g[0][i]);
            const float4 v1 = *reinterpret_cast<const float4*>(&s_g[1][i]);
            const float4 v2 = *reinterpret_cast<const float4*>(&s_g[2][i]);
            acc += (k.x == t) ? v.x : 0.f;
            acc += (k.y == t) ? v.y : 0.f;
            acc += (k.z == t) ? v.z : 0.f;
            acc += (k.w == t) ? v.w : 0.f;
            ac0 += (k.x == t) ? v0.x : 0.f;
            ac0 += (k.y == t) ? v0.y : 0.f;
            ac0 += (k.z == t) ? v0.z : 0.f;
            ac0 += (k.w == t) ? v0.w : 0.f;
            ac1 += (k.x == t) ? v1.x : 0.f;
            ac1 += (k.y == t) ? v1.y : 0.f;
            ac1 += (k.z == t) ? v1.z : 0.f;
            ac1 += (k.w == t) ? v1.w : 0.f;
            ac2 += (k.x == t) ? v2.x : 0.f;
            ac2 += (k.y == t) ? v2.y : 0.f;
            ac2 += (k.z == t) ? v2.z : 0.f;
            ac2 += (k.w == t) ? v2.w : 0.f;
        }
        part[q][0][tl] = acc;
        part[q][1][tl] = ac0;
        part[q][2][tl] = ac1;
        part[q][3][tl] = ac2;
        __syncthreads();
        if (q == 0 && t < M) {
            dsig[pass] = own.half(t, nullptr) + ((part[0][0][tl] + part[1][0][tl]) + (part[2][0][tl] + part[3][0][tl]));
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float gb = -((part[0][ch + 1][tl] + part[1][ch + 1][tl]) + (part[2][ch + 1][tl] + part[3][ch + 1][tl]));
                if (pass == 0) {
                    g_q[ch] = gb;                             // gb1_t; ga2_t joins it in pass 1
                    ga1[ch] = s_g[ch][t];                     // this target as a source: kept across the restaging
                } else {
                    g_t[ch] = ga1[ch] + gb;                   // ga1 + gb2
                    g_q[ch] = g_q[ch] + s_g[ch][t];           // gb1 + ga2
                }
            }
        }
    }
    if (q != 0 || t >= M) return;
    float g_p[3];
    {
        const float s = scale[b];
        const float* r = Rm + b * 9;
#pragma unroll
        for (int i = 0; i < 3; ++i) {                         // rigid_kernel<true>
            const float a0 = r[i] * s, a1 = r[3 + i] * s, a2 = r[6 + i] * s;
            float v = a0 * g_t[0];
            v = __builtin_fmaf(a1, g_t[1], v);
            v = __builtin_fmaf(a2, g_t[2], v);
            g_p[i] = v;
        }
    }
    const float gd = g * factor;                              // fill_scaled_kernel
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const long long row = side == 0 ? b : B + b;
        const int k = arg_on[row * M + t];
        const float dist = d_on[row * M + t];
        const float sc = dist > 0.f ? gd / dist : 0.f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float go = (kp[(row * 3 + ch) * M + t] - pc[(row * 3 + ch) * N + k]) * sc;
            g_kp[(row * 3 + ch) * M + t] = (side == 0 ? g_p[ch] : g_q[ch]) + go;
        }
    }
    g_sg[om + t] = dsig[1];
    g_sg[on + t] = dsig[0];
}

}  // namespace

extern "C" int usip_loss_tail_scan_f32(const float* keypoints, const float* R, const float* scale, const float* shift,
                                       float* kp_t, float* a, int32_t* J, float* c, int32_t* I, int B, int M,
                                       void* stream)
{
    if (B < 1 || B > 65535 || M < 1 || M > TAIL_MAX_M || !keypoints || !R || !scale || !shift || !kp_t || !a || !J ||
        !c || !I)
        return USIP_EINVAL;
    USIP_LAUNCH(loss_tail_scan_kernel, dim3(usip_ceil_div(M, 4 * ROWS), B), dim3(256), 0, (hipStream_t)stream, keypoints,
                R, scale, shift, kp_t, a, J, c, I, B, M);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_loss_tail_sums_f32(const float* a, const int32_t* J, const float* c, const int32_t* I,
                                       const float* sigmas, const float* d, float alpha, float* out6, int B, int M,
                                       void* stream)
{
    if (B < 1 || B > 65535 || M < 1 || M > TAIL_MAX_M || !a || !J || !c || !I || !sigmas || !d || !out6)
        return USIP_EINVAL;
    USIP_LAUNCH(loss_tail_sums_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a, J, c, I, sigmas, d, alpha, out6,
                B, M);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_loss_tail_backward_f32(const float* gloss, const float* keypoints, const float* sigmas,
                                           const float* kp_t, const float* a, const int32_t* J, const float* c,
                                           const int32_t* I, const float* d, const int32_t* arg, const float* pc,
                                           const float* R, const float* scale, float factor, float* g_keypoints,
                                           float* g_sigmas, int B, int M, int N, void* stream)
{
    if (B < 1 || B > 65535 || M < 1 || M > TAIL_MAX_M || N < 1 || !gloss || !keypoints || !sigmas || !kp_t || !a || !J ||
        !c || !I || !d || !arg || !pc || !R || !scale || !g_keypoints || !g_sigmas)
        return USIP_EINVAL;
    USIP_LAUNCH(loss_tail_bwd_kernel, dim3(usip_ceil_div(M, 64), B), dim3(256), 0, (hipStream_t)stream, gloss,
                keypoints, sigmas, kp_t, a, J, c, I, d, arg, pc, R, scale, factor, g_keypoints, g_sigmas, B, M, N);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
