// usip_amd/csrc/iss_walk.h -- the ASCENDING tile walk of the x-sorted baseline detectors: iss_saliency_kernel and
// iss_nms_kernel (csrc/iss.hip), harris_normals_kernel and harris_response_kernel (csrc/harris.hip), sift_dog_kernel
// (csrc/sift.hip).  A workgroup of TILE lanes owns TILE consecutive queries of a frame sorted along x (the caller's
// permutation), the frame is cut into tiles of TILE rows of that order, and the tiles that can hold a member are walked from
// low x to high x -- the order of the sums is part of these kernels' contracts, which is why they do not use tile_walk.h's
// outward walk.  Device only.
#pragma once
#include "common.h"
#include "bank.h"
#include "iss_math.h"

namespace usip_iss {

// One frame as a workgroup sees it
struct Frame {
    const float *x, *y, *z;
    const int32_t* perm;
    int n;                                                             // live points
    __device__ __forceinline__ Frame(const float* pc, const int32_t* count, const int32_t* perm_, int N, int f)
    {
        x = pc + 3LL * f * N;
        y = x + N;
        z = y + N;
        perm = perm_ + (long long)f * N;
        const int c = count ? count[f] : N;
        n = c < 0 ? 0 : (c > N ? N : c);
    }
    __device__ __forceinline__ int at(int s) const { return usip_bank::safe_index(perm[s < n ? s : n - 1], n); }   // sorted -> original
    __device__ __forceinline__ double xs(int s) const { return (double)x[at(s)]; }
    // the first tile in [0, w] whose largest x is within r of xlo (tile w is: its gap is <= 0); workgroup-uniform
    __device__ __forceinline__ int first_tile(int w, double xlo, double r) const
    {
        int lo = 0, hi = w;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (xlo - xs(mid * TILE + TILE - 1) < r) hi = mid; else lo = mid + 1;
        }
        return lo;
    }
};

// The walk the kernels share.  stage(slot, t) copies tile t of the sorted order into LDS slot `slot`; first_x(slot) is
// the x of that slot's first row; walk(slot, rows) offers its rows to the lane in ascending order.  Returns the tiles walked.
template <class Stage, class FirstX, class Walk>
__device__ __forceinline__ int walk_tiles(const Frame& F, int w, double r, bool live, Stage stage, FirstX first_x, Walk walk)
{
    const int tiles = (F.n + TILE - 1) / TILE;
    const double xlo = F.xs(w * TILE), xhi = F.xs(min(w * TILE + TILE - 1, F.n - 1));
    int seen = 0, slot = 0;
    int t = F.first_tile(w, xlo, r);
    stage(0, t);
    __syncthreads();
    while (true) {
        if (t > w && first_x(slot) - xhi >= r) break;                  // this tile and all behind it: no member
        if (t + 1 < tiles) stage(slot ^ 1, t + 1);                     // (in flight while this tile is walked)
        if (live) walk(slot, min(TILE, F.n - t * TILE));
        ++seen;
        __syncthreads();
        if (++t >= tiles) break;
        slot ^= 1;
    }
    return seen;
}

}  // namespace usip_iss
