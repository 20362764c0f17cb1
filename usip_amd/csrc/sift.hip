// usip_amd/csrc/sift.hip -- the SIFT3D baseline detector on the device: the third hand-crafted detector the
// reference compares its learned one with (evaluation/save_keypoints.py:57-61, 314-325, method = 'sift', through an external
// PCL binding).  csrc/sift_math.h has the semantics and the arithmetic, which the host twin (csrc/sift_cpu.cpp) shares.  The
// geometry is csrc/iss.hip's: pc f32 [B][3][N], count i32 [B] live points per frame, grid = (tiles of a frame, B), workgroups
// of TILE = 256 lanes.  No launch synchronises; no atomics, no float reduction across lanes, no per-lane array with a
// run-time index (the per-scale arrays are indexed by unrolled loops over the template parameter S).
//
//   sift_voxel_keys_kernel     one lane per point: the int64 key of its cell, DEAD_KEY for a dead slot or a dropped row.
//   sift_voxel_average_kernel  over the keys of a frame in ascending order (the caller's stable sort: equal keys stay in
//                              ascending input index).  A position is a HEAD when its key differs from the one before it.
//                              Every workgroup counts the heads before its tile and in the whole frame (integer sums: each
//                              lane strides over the frame's keys, then one reduction through LDS -- N / 256 loads per lane),
//                              the heads of its own tile get their rank by ballot; a head's lane sums its cell in order and
//                              writes row (heads before it).  Position s >= heads of the frame zeroes row s.  count_out[f] =
//                              heads of the frame.
//   sift_dog_kernel<S>         ascending_walk.h's kernel at a radius r with r * r >= 9 sigma_{S-1}^2, so a skipped tile
//                              holds no member of any scale and the sums are the all-pairs sums in the all-pairs order; the
//                              field rides in the float4 row's fourth component; 2 S sums in registers; dog f64 [B][S-1][N]
//                              at the cloud's own rows.
//   sift_nearest_kernel        csrc/knn_walk.h's outward walk per frame, the point itself included, one row at a time (a
//                              frame may hold non-finite rows); KList<25> in registers; idx i32 [B][N][25].
//   sift_extrema_kernel<S>     one lane per point: gathers dog at its 25 rows, minima and maxima per scale in registers;
//                              mask u8 [B][N], scale_index i32 [B][N].
// A frame with fewer than 25 points is empty for the last three.  Slots beyond count[b] get zeros.  An entry of perm or idx
// outside [0, count) reads row 0: a wrong permutation gives wrong values, never a wild read.
#include "ascending_walk.h"
#include "sift_math.h"
#include "knn_walk.h"
#include "../../include/usip_hip.h"

using namespace usip_sift;
using usip_bank::safe_index;
using usip_ascend::ascend;
using usip_ascend::Frame;
using usip_walk::nearest_rows;

namespace {

__global__ __launch_bounds__(TILE) void sift_voxel_keys_kernel(const float* __restrict__ pc, const int32_t* __restrict__ count,
                                                               int N, double leaf, int64_t* __restrict__ keys)
{
    const int f = blockIdx.y, i = blockIdx.x * TILE + threadIdx.x;
    if (i >= N) return;
    const float* x = pc + 3LL * f * N;
    const int c = count ? count[f] : N;
    keys[(long long)f * N + i] = i < c ? cell_key(x[i], x[N + i], x[2LL * N + i], leaf) : DEAD_KEY;
}

__global__ __launch_bounds__(TILE) void sift_voxel_average_kernel(const float* __restrict__ pc, const float* __restrict__ field,
                                                                  int axis, const int64_t* __restrict__ keys,
                                                                  const int32_t* __restrict__ order, int N,
                                                                  float* __restrict__ out_pc, float* __restrict__ out_field,
                                                                  int32_t* __restrict__ count_out)
{
    __shared__ int32_t sums[3][TILE / 64];
    const int l = threadIdx.x, w = blockIdx.x, f = blockIdx.y, q = w * TILE + l;
    const float *x = pc + 3LL * f * N, *y = x + N, *z = y + N;
    const float* fl = field ? field + (long long)f * N : nullptr;
    const int64_t* k = keys + (long long)f * N;
    const int32_t* ord = order + (long long)f * N;
    const auto head = [&](int s) { return s < N && k[s] != DEAD_KEY && (s == 0 || k[s] != k[s - 1]); };
    int before = 0, total = 0;
    for (int t = 0; t * TILE < N; ++t) {                               // (workgroup-uniform trip count)
        const int h = head(t * TILE + l) ? 1 : 0;
        total += h;
        before += t < w ? h : 0;
    }
    const bool mine = head(q);
    const unsigned long long vote = __ballot(mine);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        before += __shfl_xor(before, off);
        total += __shfl_xor(total, off);
    }
    if ((l & 63) == 0) {
        sums[0][l >> 6] = before;
        sums[1][l >> 6] = total;
        sums[2][l >> 6] = __popcll(vote);
    }
    __syncthreads();
    before = 0;
    total = 0;
    int rank = usip_mbcnt(vote);
#pragma unroll
    for (int v = 0; v < TILE / 64; ++v) {
        before += sums[0][v];
        total += sums[1][v];
        rank += v < (l >> 6) ? sums[2][v] : 0;
    }
    float *ox = out_pc + 3LL * f * N, *oy = ox + N, *oz = oy + N, *of = out_field + (long long)f * N;
    if (mine) {
        CellSum cell;
        const int64_t key = k[q];
        for (int s = q; s < N && k[s] == key; ++s) {
            const int j = safe_index(ord[s], N);
            cell.add(x[j], y[j], z[j], fl ? fl[j] : 0.0f);
        }
        const int row = before + rank;                                 // < total <= N
        cell.centroid(fl != nullptr, axis, ox + row, oy + row, oz + row, of + row);
    }
    if (q < N && q >= total) {
        ox[q] = 0.0f;
        oy[q] = 0.0f;
        oz[q] = 0.0f;
        of[q] = 0.0f;
    }
    if (q == 0) count_out[f] = total;
}

template <int S>
struct DogPass : usip_ascend::Plain {
    static constexpr int ROWS = 1;
    const Scales& sc;
    const float* fl;
    double* out;
    int N;
    ScaleSums<S> g;
    USIP_DEV float stage(int, int, int j) const { return fl[j]; }      // the field rides in the row's fourth component
    USIP_DEV void offer(double xi, double yi, double zi, float4 o, Side) { g.offer(xi, yi, zi, o.x, o.y, o.z, o.w, sc); }
    USIP_DEV void dead(int q) const
    {
#pragma unroll
        for (int s = 0; s + 1 < S; ++s) out[(long long)s * N + q] = 0.0;
    }
    USIP_DEV void write(int me, double, double, double) const { g.dog(out + me, N); }
};

template <int S>
__global__ __launch_bounds__(TILE) void sift_dog_kernel(const float* __restrict__ pc, const float* __restrict__ field,
                                                        const int32_t* __restrict__ count, const int32_t* __restrict__ perm,
                                                        int N, Scales sc, double r, double* __restrict__ dog,
                                                        int32_t* __restrict__ visited)
{
    __shared__ float4 tile[2][TILE];
    const int f = blockIdx.y;
    Frame F(pc, count, perm, N, f);
    F.n = F.n < MIN_POINTS ? 0 : F.n;
    DogPass<S> pass{{}, sc, field + (long long)f * N, dog + (long long)f * (S - 1) * N, N};
    pass.g.clear();
    ascend(F, N, r, tile, visited, pass);
}

__global__ __launch_bounds__(TILE) void sift_nearest_kernel(const float* __restrict__ pc, const int32_t* __restrict__ count,
                                                            const int32_t* __restrict__ perm, int N, int32_t* __restrict__ idx)
{
    __shared__ float4 tile[2][TILE];
    __shared__ int32_t orig[2][TILE];
    __shared__ double slots[4];
    const int l = threadIdx.x, b = blockIdx.x, f = blockIdx.y;
    Frame F(pc, count, perm, N, f);
    F.n = F.n < MIN_POINTS ? 0 : F.n;
    const int q = b * TILE + l;                                        // position in the sorted order
    int32_t* out = idx + (long long)f * N * NEAREST;
    if (q >= F.n && q < N) {
#pragma unroll
        for (int k = 0; k < NEAREST; ++k) out[(long long)q * NEAREST + k] = 0;
    }
    if (b * TILE >= F.n) return;                                       // workgroup-uniform: no query here
    nearest_rows<NEAREST, true, false>(F, b, tile, orig, slots, out);
}

template <int S>
__global__ __launch_bounds__(TILE) void sift_extrema_kernel(const double* __restrict__ dog, const int32_t* __restrict__ idx,
                                                            const int32_t* __restrict__ count, int N, double min_contrast,
                                                            uint8_t* __restrict__ mask, int32_t* __restrict__ scale_index)
{
    const int f = blockIdx.y, i = blockIdx.x * TILE + threadIdx.x;
    if (i >= N) return;
    const int n = octave_points(count, f, N);
    const double* d = dog + (long long)f * (S - 1) * N;
    const int32_t* nb = idx + ((long long)f * N + i) * NEAREST;
    int found = 0;
    if (i < n) {
        Extrema<S> e;
        e.clear();
        for (int k = 0; k < NEAREST; ++k) e.offer(d + safe_index(nb[k], n), N);
        found = e.decide(d + i, N, min_contrast);
    }
    mask[(long long)f * N + i] = found ? 1 : 0;
    scale_index[(long long)f * N + i] = found;
}

}  // namespace

extern "C" int usip_sift_voxel_keys_f32(const float* pc, const int32_t* count, int B, int N, double leaf, int64_t* keys,
                                        void* stream)
{
    if (bad_frames(B, N) || !(leaf > 0.0) || !is_finite(leaf) || !pc || !keys) return USIP_EINVAL;
    USIP_LAUNCH(sift_voxel_keys_kernel, dim3(usip_ceil_div(N, TILE), B), dim3(TILE), 0, (hipStream_t)stream, pc, count, N, leaf,
                keys);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_sift_voxel_average_f32(const float* pc, const float* field, int axis, const int64_t* sorted_keys,
                                           const int32_t* order, int B, int N, float* out_pc, float* out_field,
                                           int32_t* count_out, void* stream)
{
    if (bad_frames(B, N) || axis < 0 || axis > 2 || !pc || !sorted_keys || !order || !out_pc || !out_field || !count_out)
        return USIP_EINVAL;
    USIP_LAUNCH(sift_voxel_average_kernel, dim3(usip_ceil_div(N, TILE), B), dim3(TILE), 0, (hipStream_t)stream, pc, field, axis,
                sorted_keys, order, N, out_pc, out_field, count_out);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_sift_dog_f32(const float* pc, const float* field, const int32_t* count, const int32_t* perm, int B, int N,
                                 int S, const double* sigma2, double* dog, int32_t* tiles_visited, void* stream)
{
    if (bad_frames(B, N) || !good_scales(sigma2, S) || !pc || !field || !perm || !dog) return USIP_EINVAL;
    const Scales sc = make_scales(sigma2, S);
    const double r = walk_radius(sc.bound(S - 1));
#define USIP_SIFT_DOG(s)                                                                                                       \
    USIP_LAUNCH(sift_dog_kernel<s>, dim3(usip_ceil_div(N, TILE), B), dim3(TILE), 0, (hipStream_t)stream, pc, field, count, perm, \
                N, sc, r, dog, tiles_visited)
    USIP_SIFT_DISPATCH(S, USIP_SIFT_DOG)
#undef USIP_SIFT_DOG
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_sift_nearest_f32(const float* pc, const int32_t* count, const int32_t* perm, int B, int N, int32_t* idx,
                                     void* stream)
{
    if (bad_frames(B, N) || !pc || !perm || !idx) return USIP_EINVAL;
    USIP_LAUNCH(sift_nearest_kernel, dim3(usip_ceil_div(N, TILE), B), dim3(TILE), 0, (hipStream_t)stream, pc, count, perm, N,
                idx);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_sift_extrema_f32(const double* dog, const int32_t* idx, const int32_t* count, int B, int N, int S,
                                     double min_contrast, uint8_t* mask, int32_t* scale_index, void* stream)
{
    if (bad_frames(B, N) || S < SCALES_MIN || S > SCALES_MAX || !(min_contrast >= 0.0) || !dog || !idx || !mask || !scale_index)
        return USIP_EINVAL;
#define USIP_SIFT_EXTREMA(s)                                                                                                  \
    USIP_LAUNCH(sift_extrema_kernel<s>, dim3(usip_ceil_div(N, TILE), B), dim3(TILE), 0, (hipStream_t)stream, dog, idx, count, N, \
                min_contrast, mask, scale_index)
    USIP_SIFT_DISPATCH(S, USIP_SIFT_EXTREMA)
#undef USIP_SIFT_EXTREMA
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
