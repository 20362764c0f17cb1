// usip_amd/csrc/cgf_loss.hip -- the CGF triplet loss of the indoor descriptor on the device (the reference's
// losses.DescCGFLoss, models/losses.py:240-314).  csrc/cgf_math.h has the semantics and the arithmetic, which the host twin
// (csrc/cgf_loss_cpu.cpp) shares.  Keypoints f32 [B][3][M], descriptors f32 [B][C][M], sigmas f32 [B][M].  The reference
// materialises a B x C x M x M difference tensor, a B x M x M norm and three random B x M x M matrices and then reads three
// entries per anchor; here no M x M array exists (the explicit draws of the tests apart).  No launch synchronises the host;
// no floating-point atomics; every index read back from memory is clamped; no per-lane array with a run-time index.
//
//   cgf_select_kernel    grid B * ceil(M / 4) (a workgroup per four anchors of one batch element; beyond MAX_GRID workgroups
//                        every kernel here loops), 256 lanes, one wave per anchor.  The workgroup stages the batch element's
//                        positive keypoints through LDS, CHUNK at a time (12 KB); lane l offers the candidates l, l + 64, ...
//                        of every chunk to its three running picks; a butterfly over the wave merges them (Picks::merge is
//                        symmetric and its order total, so every lane ends with the row's answer).  Every wave reaches every
//                        barrier: an idle wave of the last workgroup stages and offers nothing.
//   cgf_dist_kernel      the same grid without LDS: lane l adds channels l, l + 64, ... of the two squared distances, the
//                        binary tree runs on shuffles (lane l takes lane l + s, s = 32 .. 1: lane 0 holds the tree's root).
//   cgf_row_kernel       one workgroup of 256 per batch element: strided partial sums, the tree through LDS, the row.
//   cgf_backward_kernel  the first grid again: wave (b, w) writes d_anc's column w, then d_pos's column w.  For the latter its
//                        lanes test 64 anchors at a time against the column, and the wave walks the matches of the ballot in
//                        ascending anchor order, the positive term of an anchor before its negative one -- the column's
//                        ordered sum without an atomic.  Lanes hold channels, 64 at a time.
// A [C][M] tensor makes a column a strided read; at 256 KB per tensor the L2 serves it.
#include "common.h"
#include "cgf_math.h"

using namespace usip_cgf;

namespace {

constexpr int TILE = 256;
constexpr int WAVES = TILE / LANES;
constexpr int CHUNK = 1024;
constexpr long long MAX_GRID = 1LL << 22;        // workgroups of a launch; the kernels loop beyond it

__device__ __forceinline__ void butterfly(Picks& k)
{
#pragma unroll
    for (int off = LANES / 2; off >= 1; off >>= 1) {
        Picks o;
        o.pos.key = __shfl_xor(k.pos.key, off, LANES); o.pos.j = __shfl_xor(k.pos.j, off, LANES);
        o.far.key = __shfl_xor(k.far.key, off, LANES); o.far.j = __shfl_xor(k.far.j, off, LANES);
        o.out.key = __shfl_xor(k.out.key, off, LANES); o.out.j = __shfl_xor(k.out.j, off, LANES);
        o.has = __shfl_xor((int)k.has, off, LANES) != 0;
        k.merge(o);
    }
}

__global__ __launch_bounds__(TILE) void cgf_select_kernel(const float* __restrict__ anc_kp, const float* __restrict__ pos_kp,
                                                          long long blocks, int M, float r, const float* __restrict__ u1,
                                                          const float* __restrict__ u2, const float* __restrict__ u3,
                                                          uint64_t seed, uint64_t step, const uint64_t* __restrict__ step_dev,
                                                          uint64_t elem_base, int32_t* __restrict__ sel,
                                                          uint8_t* __restrict__ has, uint8_t* __restrict__ take_far)
{
    __shared__ float px[CHUNK], py[CHUNK], pz[CHUNK];
    const int lane = threadIdx.x & (LANES - 1), wave = threadIdx.x >> 6, tiles = (M + WAVES - 1) / WAVES;
    const bool drawn = u1 == nullptr;                                  // kernel-uniform
    const uint64_t st = step_dev ? *step_dev : step;
    for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) { // one turn, unless B * tiles outgrows a grid
        const long long b = blk / tiles;
        const int i = (int)(blk % tiles) * WAVES + wave;               // the wave's anchor
        const bool there = i < M;                                      // wave-uniform
        const float* A = anc_kp + 3 * b * M;
        const float* P = pos_kp + 3 * b * M;
        const float ax = there ? A[i] : 0.f, ay = there ? A[M + i] : 0.f, az = there ? A[2LL * M + i] : 0.f;
        const uint64_t gelem = elem_base + (uint64_t)b;
        const long long at = b * M + i, row = at * M;                  // row: of the explicit draws
        Picks k;
        k.init();
        for (int base = 0; base < M; base += CHUNK) {
            const int n = M - base < CHUNK ? M - base : CHUNK;
            __syncthreads();                                           // the previous chunk has been read
            for (int t = threadIdx.x; t < n; t += TILE) {
                px[t] = P[base + t];
                py[t] = P[M + base + t];
                pz[t] = P[2LL * M + base + t];
            }
            __syncthreads();
            if (there)
                for (int t = lane; t < n; t += LANES) {
                    const int j = base + t;
                    float a1, a2;
                    if (drawn) draw_pair(seed, st, gelem, i, j, a1, a2);
                    else { a1 = u1[row + j]; a2 = u2[row + j]; }
                    k.offer(ax, ay, az, px[t], py[t], pz[t], r, a1, a2, j);
                }
        }
        if (!there) continue;                                          // (its barriers are behind it)
        butterfly(k);
        if (lane == 0) {
            sel[3 * at] = picked(k.pos);
            sel[3 * at + 1] = picked(k.far);
            sel[3 * at + 2] = picked(k.out);
            has[at] = k.has ? 1 : 0;
            take_far[at] = takes_far(drawn ? draw_anchor(seed, st, gelem, i) : u3[at]) ? 1 : 0;
        }
    }
}

// the anchor's two partners, clamped: (j_pos, j_neg)
__device__ __forceinline__ void partners(const int32_t* __restrict__ sel, const uint8_t* __restrict__ take_far, long long at, int M,
                                         int& jp, int& jn)
{
    jp = clamp_index(sel[3 * at], M);
    jn = clamp_index(take_far[at] ? sel[3 * at + 1] : sel[3 * at + 2], M);
}

__global__ __launch_bounds__(TILE) void cgf_dist_kernel(const float* __restrict__ anc_desc, const float* __restrict__ pos_desc,
                                                        const int32_t* __restrict__ sel, const uint8_t* __restrict__ take_far,
                                                        long long blocks, int M, int C, double* __restrict__ dist)
{
    const int lane = threadIdx.x & (LANES - 1), wave = threadIdx.x >> 6, tiles = (M + WAVES - 1) / WAVES;
    for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
        const long long b = blk / tiles;
        const int i = (int)(blk % tiles) * WAVES + wave;
        if (i >= M) continue;                                          // wave-uniform; the kernel has no barrier
        const long long at = b * M + i;
        int jp, jn;
        partners(sel, take_far, at, M, jp, jn);
        const float* A = anc_desc + b * C * M;
        const float* P = pos_desc + b * C * M;
        double sp = 0.0, sn = 0.0;
        for (int c = lane; c < C; c += LANES) {
            const float a = A[(long long)c * M + i];
            sp += sqdiff(a, P[(long long)c * M + jp]);
            sn += sqdiff(a, P[(long long)c * M + jn]);
        }
#pragma unroll
        for (int s = LANES / 2; s >= 1; s >>= 1) {
            sp += __shfl_down(sp, s, LANES);
            sn += __shfl_down(sn, s, LANES);
        }
        if (lane == 0) {
            dist[2 * at] = sqrt(sp);
            dist[2 * at + 1] = sqrt(sn);
        }
    }
}

__global__ __launch_bounds__(ROW_LANES) void cgf_row_kernel(const float* __restrict__ anc_sigma, const uint8_t* __restrict__ has,
                                                            const double* __restrict__ dist, int B, int M, double gamma,
                                                            double sigma_max, float* __restrict__ loss,
                                                            float* __restrict__ active, double* __restrict__ coef)
{
    __shared__ double part[ROW_LANES];
    __shared__ int matched[ROW_LANES], live[ROW_LANES];
    const int l = threadIdx.x;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {                  // one turn, unless B outgrows a grid
        const long long row = (long long)b * M;
        double w = 0.0;
        int n = 0, act = 0;
        for (int i = l; i < M; i += ROW_LANES) {
            const bool h = has[row + i] != 0;
            w += raw_weight(sigma_max, anc_sigma[row + i]);
            n += h ? 1 : 0;
            act += before_clamp(h, dist[2 * (row + i)], dist[2 * (row + i) + 1], gamma) > ACTIVE_EPS ? 1 : 0;
        }
        part[l] = w;
        matched[l] = n;
        live[l] = act;
        for (int s = ROW_LANES / 2; s > 0; s >>= 1) {
            __syncthreads();
            if (l < s) {
                part[l] += part[l + s];
                matched[l] += matched[l + s];
                live[l] += live[l + s];
            }
        }
        __syncthreads();
        const double mean = part[0] / (double)M;
        const int n1 = matched[0] + 1;
        if (l == 0) active[b] = (float)((double)live[0] / (double)n1);
        for (int i = l; i < M; i += ROW_LANES) {
            const bool h = has[row + i] != 0;
            const double before = before_clamp(h, dist[2 * (row + i)], dist[2 * (row + i) + 1], gamma);
            row_values(raw_weight(sigma_max, anc_sigma[row + i]), mean, before, M, n1, coef[row + i], loss[row + i]);
        }
        __syncthreads();                                               // the sums have been read
    }
}

__global__ __launch_bounds__(TILE) void cgf_backward_kernel(const float* __restrict__ anc_desc, const float* __restrict__ pos_desc,
                                                            const int32_t* __restrict__ sel, const uint8_t* __restrict__ take_far,
                                                            const double* __restrict__ dist, const double* __restrict__ coef,
                                                            const float* __restrict__ grad_loss, long long blocks, int M, int C,
                                                            float* __restrict__ d_anc, float* __restrict__ d_pos)
{
    const int lane = threadIdx.x & (LANES - 1), wave = threadIdx.x >> 6, tiles = (M + WAVES - 1) / WAVES;
    for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
        const long long b = blk / tiles;
        const int w = (int)(blk % tiles) * WAVES + wave;               // the wave's anchor, then its column
        if (w >= M) continue;                                          // wave-uniform; the kernel has no barrier
        const long long row = b * M;
        const float* A = anc_desc + b * C * M;
        const float* P = pos_desc + b * C * M;
        float* dA = d_anc + b * C * M;
        float* dP = d_pos + b * C * M;
        {
            int jp, jn;
            partners(sel, take_far, row + w, M, jp, jn);
            const double g = (double)grad_loss[row + w] * coef[row + w];
            const double Dp = dist[2 * (row + w)], Dn = dist[2 * (row + w) + 1];
            for (int c = lane; c < C; c += LANES) {
                const float a = A[(long long)c * M + w];
                dA[(long long)c * M + w] =
                    (float)(g * (unit(a, P[(long long)c * M + jp], Dp) - unit(a, P[(long long)c * M + jn], Dn)));
            }
        }
        for (int cb = 0; cb < C; cb += LANES) {
            const int c = cb + lane;
            const bool mine = c < C;
            const float p = mine ? P[(long long)c * M + w] : 0.f;
            double acc = 0.0;
            for (int base = 0; base < M; base += LANES) {
                const int t = base + lane;
                bool mp = false, mn = false;
                if (t < M) {
                    int jp, jn;
                    partners(sel, take_far, row + t, M, jp, jn);
                    mp = jp == w;
                    mn = jn == w;
                }
                const unsigned long long bp = __ballot(mp), bn = __ballot(mn);
                unsigned long long both = bp | bn;
                while (both) {                                         // wave-uniform: ascending anchors
                    const int s = __ffsll((long long)both) - 1;
                    both &= both - 1;
                    const int i = base + s;
                    const double g = (double)grad_loss[row + i] * coef[row + i];
                    if (mine) {
                        const float a = A[(long long)c * M + i];
                        if ((bp >> s) & 1ull) acc -= g * unit(a, p, dist[2 * (row + i)]);
                        if ((bn >> s) & 1ull) acc += g * unit(a, p, dist[2 * (row + i) + 1]);
                    }
                }
            }
            if (mine) dP[(long long)c * M + w] = (float)acc;
        }
    }
}

}  // namespace

extern "C" int usip_cgf_select_f32(const float* anc_kp, const float* pos_kp, int B, int M, double radius, const float* u1,
                                   const float* u2, const float* u3, uint64_t seed, uint64_t step, const uint64_t* step_dev,
                                   uint64_t elem_base, int32_t* sel, uint8_t* has, uint8_t* take_far, void* stream)
{
    const bool some = u1 || u2 || u3, all = u1 && u2 && u3;
    if (bad_shape(B, M) || bad_radius(radius) || !anc_kp || !pos_kp || !sel || !has || !take_far || some != all)
        return USIP_EINVAL;
    const long long blocks = (long long)B * usip_ceil_div(M, WAVES);
    const dim3 grid((unsigned)(blocks < MAX_GRID ? blocks : MAX_GRID)), block(TILE);
    USIP_LAUNCH(cgf_select_kernel, grid, block, 0, (hipStream_t)stream, anc_kp, pos_kp, blocks, M, (float)radius, u1, u2, u3, seed, step,
                step_dev, elem_base, sel, has, take_far);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_cgf_loss_f32(const float* anc_desc, const float* pos_desc, const float* anc_sigma, const int32_t* sel,
                                 const uint8_t* has, const uint8_t* take_far, int B, int M, int C, double gamma,
                                 double sigma_max, float* loss, float* active, double* dist, double* coef, void* stream)
{
    if (bad_shape(B, M) || bad_channels(C) || !anc_desc || !pos_desc || !anc_sigma || !sel || !has || !take_far ||
        !loss || !active || !dist || !coef)
        return USIP_EINVAL;
    const long long blocks = (long long)B * usip_ceil_div(M, WAVES);
    const dim3 grid((unsigned)(blocks < MAX_GRID ? blocks : MAX_GRID)), block(TILE);
    USIP_LAUNCH(cgf_dist_kernel, grid, block, 0, (hipStream_t)stream, anc_desc, pos_desc, sel, take_far, blocks, M, C, dist);
    USIP_LAUNCH_CHECK();
    USIP_LAUNCH(cgf_row_kernel, dim3((unsigned)(B < MAX_GRID ? B : MAX_GRID)), dim3(ROW_LANES), 0, (hipStream_t)stream, anc_sigma, has,
                (const double*)dist, B, M, gamma,
                sigma_max, loss, active, coef);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_cgf_loss_backward_f32(const float* anc_desc, const float* pos_desc, const int32_t* sel, const uint8_t* take_far,
                                          const double* dist, const double* coef, const float* grad_loss, int B, int M, int C,
                                          float* d_anc, float* d_pos, void* stream)
{
    if (bad_shape(B, M) || bad_channels(C) || !anc_desc || !pos_desc || !sel || !take_far || !dist || !coef ||
        !grad_loss || !d_anc || !d_pos)
        return USIP_EINVAL;
    const long long blocks = (long long)B * usip_ceil_div(M, WAVES);
    const dim3 grid((unsigned)(blocks < MAX_GRID ? blocks : MAX_GRID)), block(TILE);
    USIP_LAUNCH(cgf_backward_kernel, grid, block, 0, (hipStream_t)stream, anc_desc, pos_desc, sel, take_far, dist, coef, grad_loss,
                blocks, M, C, d_anc, d_pos);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
