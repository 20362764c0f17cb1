// usip_amd/csrc/tile_walk.h -- the outward tile walk of the x-sorted neighbour searches: overlap_kernel<XQ>
// (csrc/fragments.hip, existence within a radius), icp_nearest_kernel (csrc/icp.hip, the exact nearest row) and
// csrc/knn_walk.h's nearest_rows (the K nearest within one cloud: scan_knn_kernel<K> of csrc/prepare.hip and sift_nearest_kernel
// of csrc/sift.hip, over Tiles and block_minmax).  A workgroup of 256 lanes owns 256 queries; the database, sorted along x, is cut into
// tiles of 256 rows; two of them are staged in LDS per round, one to either side of the start tile, every lane walks both at
// the same LDS address, and a side ends once the x-gap to its next tile alone rules that tile out.  What a tile holds in LDS,
// the per-row test and the rule that ends a side are the kernel's own (its stage, visit and prune); the order of the rounds,
// the start tile, the x at a tile's near edge with the partial last tile clamped, and the workgroup's smallest / largest x
// are here.  Device only.
// csrc/ascending_walk.h's walk_tiles (csrc/iss.hip, csrc/harris.hip, csrc/sift.hip's scale space) is not one of these: it
// walks ascending because the order of its sums is part of those kernels' contracts.
#pragma once
#include <hip/hip_runtime.h>

namespace usip_walk {

constexpr int WALK_TILE = 256;               // lanes of the workgroup = queries = database rows per LDS tile
constexpr int WALK_WAVES = WALK_TILE / 64;

// The smallest (LO) and / or the largest (HI) v of the workgroup, in every lane; slots: WALK_WAVES doubles per result asked for.
// One barrier.  A caller that comes back while lanes may still read the slots puts its own barrier in front.
template <bool LO, bool HI>
__device__ __forceinline__ void block_minmax(double& lo, double& hi, double* slots)
{
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        if (LO) { const double a = __shfl_xor(lo, off); lo = a < lo ? a : lo; }
        if (HI) { const double b = __shfl_xor(hi, off); hi = b > hi ? b : hi; }
    }
    if ((threadIdx.x & 63) == 0) {
        if (LO) slots[w] = lo;
        if (HI) slots[(LO ? WALK_WAVES : 0) + w] = hi;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < WALK_WAVES; ++k) {
        if (LO) { const double a = slots[k]; lo = k == 0 || a < lo ? a : lo; }
        if (HI) { const double b = slots[(LO ? WALK_WAVES : 0) + k]; hi = k == 0 || b > hi ? b : hi; }
    }
}

// The tiles of n >= 1 rows sorted along x; x_at(s) is the x of the row at sorted position s < n.
template <class XAt>
struct Tiles {
    int n, tiles;
    XAt x_at;
    __device__ __forceinline__ Tiles(int n_, XAt x) : n(n_), tiles((n_ + WALK_TILE - 1) / WALK_TILE), x_at(x) {}
    // the tile of the first sorted position whose x is not below xlo (the last tile when there is none)
    __device__ __forceinline__ int start(double xlo) const
    {
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (x_at(mid) < xlo) lo = mid + 1; else hi = mid;
        }
        return min(lo / WALK_TILE, tiles - 1);
    }
    // x of tile t's row nearest to the start: its last row seen from the right (side 0), its first from the left (side 1)
    __device__ __forceinline__ double near_x(int side, int t) const
    {
        return x_at(side == 0 ? min(t * WALK_TILE + WALK_TILE - 1, n - 1) : t * WALK_TILE);
    }
    __device__ __forceinline__ int rows(int t) const { return min(WALK_TILE, n - t * WALK_TILE); }
};

// Rounds until both sides have ended (left < 0, right >= tiles).  prune(left, right) -> END_LEFT | END_RIGHT, workgroup-
// uniform, holds the kernel's barriers and may end either side or both; stage(side, t) writes tile t into LDS slot `side`; one
// barrier; visit(side, t, rows of tile t) runs per lane; then both sides step outward.
// csrc/knn_walk.h's nearest_rows writes these same rounds out in its own body, over Tiles and block_minmax: its K-list of 3 K
// registers is live across the whole walk, and with the rounds behind this function's boundary hipcc (ROCm 7.2) allocates 144
// VGPRs at K = 16 where the loop in place takes 126 of the 128 that four waves per SIMD allow (tests/test_prepare_isa.py).
constexpr int END_LEFT = 1, END_RIGHT = 2;

template <class XAt, class Prune, class Stage, class Visit>
__device__ __forceinline__ void walk_outward(const Tiles<XAt>& tiles, int left, int right, Prune prune, Stage stage,
                                             Visit visit)
{
    while (true) {
        const int ended = prune(left, right);
        if (ended & END_LEFT) left = -1;
        if (ended & END_RIGHT) right = tiles.tiles;
        if (left < 0 && right >= tiles.tiles) break;
        if (left >= 0) stage(0, left);
        if (right < tiles.tiles) stage(1, right);
        __syncthreads();
        if (left >= 0) visit(0, left, tiles.rows(left));
        if (right < tiles.tiles) visit(1, right, tiles.rows(right));
        if (left >= 0) --left;
        if (right < tiles.tiles) ++right;
    }
}

}  // namespace usip_walk
