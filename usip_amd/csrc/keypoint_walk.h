// usip_amd/csrc/keypoint_walk.h -- the WAVE-PER-KEYPOINT walk of the x-sorted baseline descriptors and the kernel body around
// its LDS-histogram form: fpfh_gather_kernel (csrc/fpfh.hip), shot_lrf_kernel and shot_hist_kernel (csrc/shot.hip),
// spin_image_kernel<S> (csrc/spin.hip).  grid = (ceil(M / 4), B), TILE = 256 lanes: wave w of workgroup g owns keypoint
// q = 4 g + w of frame blockIdx.y, at any position.  The wave finds [lo, hi), the positions of the frame sorted along x (the
// caller's permutation) with |x - q_x| < r, by two binary searches (wave-uniform): a row before lo has fl(q_x - x) >= r and a row
// from hi on has fl(x - q_x) >= r, so dx of sqdist has |dx| >= r and d2 >= fl(dx dx) >= fl(r r) = r2 (float64 rounding is
// monotone): no member, and the result is the all-pairs answer.  Lane l takes the rows lo + l + 64 k, ascending, and lanes fold
// by the xor-butterfly 32 .. 1: where a sum is float64 that order is the contract (csrc/keypoints_host.h has the twins' side of
// it).  Keypoint is the wave's keypoint, Window its [lo, hi), walk() the row loop, fold() the butterfly.  Device only.
//
// histogram(F, ..., bins, hist, desc, kp_members, pass) is the whole kernel behind its arguments for the two kernels that sum
// integers into a per-wave LDS row, u64 bins[TILE / LANES][WIDTH]: the wave zeroes its row; barrier; it walks, and a lane adds
// what its members add with LDS 64-bit integer atomic adds (integer sums: the order is free); barrier (the waves of a workgroup
// are independent: the two barriers are more than the wave-level ordering this needs, cost nothing measurable, and every wave
// reaches them -- an idle wave of the last workgroup walks nothing); k = fold(k); lane l reads the columns l + 64 i and writes
// them to hist i64 [B][M][WIDTH] and, finished by the pass, to desc f64 [B][M][WIDTH] (a wave's 64 lanes write 64 consecutive
// columns at a time); lane 0 writes kp_members i32 [B][M].  A PASS is what one kernel does on the way:
//   WIDTH                       columns of a row
//   Key, load(q)                what the keypoint reads beside its coordinates (SHOT's frame, spin's axis)
//   walks(key)                  whether the keypoint walks at all (wave-uniform)
//   offer(key, K, j, xj, yj, zj, d2, k, add)   one row: the member test, ++k, and add(column, quanta) for what it adds
//   finish(h, lane)             sees the lane's columns before they leave (SHOT's sum of squares: every lane calls it)
//   column(h, k)                a column's float64 value
// Slots beyond kp_count[b] get zeros.
#pragma once
#include "ascending_walk.h"
#include "fpfh_math.h"

namespace usip_keypoint {

using usip_ascend::Frame;
using usip_fpfh::first_within;
using usip_fpfh::LANES;
using usip_iss::TILE;

template <class T>
USIP_DEV T fold(T v)
{
#pragma unroll
    for (int off = LANES / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, LANES);
    return v;
}

// The wave's keypoint
struct Keypoint {
    int f, lane, wave, q;
    bool there, live;                                                  // wave-uniform: q < M; and live, in a frame with a row to read
    double x = 0.0, y = 0.0, z = 0.0;                                  // of one that is there
    USIP_DEV Keypoint(const Frame& F, const float* keypoints, const int32_t* kp_count, int M)
        : f(blockIdx.y), lane(threadIdx.x & (LANES - 1)), wave(threadIdx.x >> 6), q(blockIdx.x * (TILE / LANES) + wave),
          there(q < M), live(there && q < usip_iss::live_points(kp_count, f, M) && F.n > 0)
    {
        if (!there) return;
        const float* kp = keypoints + 3LL * f * M;
        x = (double)kp[q];
        y = (double)kp[M + q];
        z = (double)kp[2LL * M + q];
    }
    USIP_DEV long long slot(int M) const { return (long long)f * M + q; }   // its row of an output [B][M][..]
};

// [lo, hi) of the sorted positions that can hold a member of the keypoint; empty for one that is not live; wave-uniform
struct Window {
    int lo = 0, hi = 0;
    USIP_DEV Window(const Frame& F, const Keypoint& K, double r)
    {
        if (!K.live) return;
        const auto xs = [&](int s) { return F.xs(s); };
        lo = first_within(F.n, K.x, r, xs);
        hi = lo;
        int end = F.n;                                                 // the first position from lo on with x - q_x >= r
        while (hi < end) {
            const int mid = (hi + end) >> 1;
            if (xs(mid) - K.x >= r) end = mid; else hi = mid + 1;
        }
    }
};

// fn(j, xj, yj, zj, d2) for the lane's rows of the window, ascending: original index, coordinates, sqdist from the keypoint
template <class Fn>
USIP_DEV void walk(const Frame& F, const Window& W, const Keypoint& K, Fn fn)
{
    for (int s = W.lo + K.lane; s < W.hi; s += LANES) {
        const int j = F.at(s);
        const float xj = F.x[j], yj = F.y[j], zj = F.z[j];
        fn(j, xj, yj, zj, usip_prep::sqdist(K.x, K.y, K.z, xj, yj, zj));
    }
}

template <class Pass>
USIP_DEV void histogram(const Frame& F, const float* keypoints, const int32_t* kp_count, int M, double r,
                        unsigned long long (*bins)[Pass::WIDTH], long long* hist, double* desc, int32_t* kp_members, Pass& pass)
{
    constexpr int WIDTH = Pass::WIDTH, PER_LANE = (WIDTH + LANES - 1) / LANES;
    unsigned long long* mine = bins[threadIdx.x >> 6];
    for (int c = threadIdx.x & (LANES - 1); c < WIDTH; c += LANES) mine[c] = 0ULL;
    __syncthreads();
    const Keypoint K(F, keypoints, kp_count, M);
    int32_t k = 0;
    if (K.live) {                                                      // wave-uniform
        const typename Pass::Key key = pass.load(K.q);
        if (pass.walks(key))                                           // wave-uniform
            walk(F, Window(F, K, r), K, [&](int j, float xj, float yj, float zj, double d2) {
                pass.offer(key, K, j, xj, yj, zj, d2, k,
                           [&](int column, long long quanta) { atomicAdd(&mine[column], (unsigned long long)quanta); });
            });
    }
    __syncthreads();
    if (!K.there) return;
    k = fold(k);
    long long h[PER_LANE];
#pragma unroll
    for (int i = 0; i < PER_LANE; ++i) h[i] = K.lane + LANES * i < WIDTH ? (long long)mine[K.lane + LANES * i] : 0LL;
    pass.finish(h, K.lane);
    long long* hrow = hist + WIDTH * K.slot(M);
    double* drow = desc + WIDTH * K.slot(M);
#pragma unroll
    for (int i = 0; i < PER_LANE; ++i) {
        const int c = K.lane + LANES * i;
        if (c < WIDTH) {
            hrow[c] = h[i];
            drow[c] = pass.column(h[i], k);
        }
    }
    if (K.lane == 0) kp_members[K.slot(M)] = k;
}

}  // namespace usip_keypoint
