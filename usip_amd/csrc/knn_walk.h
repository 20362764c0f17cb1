// usip_amd/csrc/knn_walk.h -- the K nearest rows of every row of one x-sorted cloud, over tile_walk.h's tiles: the body of
// scan_knn_kernel<K> (csrc/prepare.hip) and sift_nearest_kernel (csrc/sift.hip).  A workgroup owns TILE = 256 consecutive
// queries of the cloud SORTED ALONG X (the caller's permutation), one lane per query, its K-list (float64 d2, int32 index) in
// registers.  Database tiles of 256 rows are staged in LDS as 16-byte rows beside their original indices and walked by every
// lane at the same address (broadcast reads).  The walk starts at the workgroup's own tile and goes outward in both directions;
// a direction ends once the squared x-gap between its next tile and the workgroup's query range exceeds the largest K-th
// distance any lane still holds (a workgroup-wide max through LDS).  Every point of a skipped tile has d2 >= fl(gap * gap) >
// that K-th distance for every lane (float64 rounding is monotone), so it could not have entered any list: the result is the
// all-pairs answer, ties on ORIGINAL indices included.  Device only.
//
// The rounds are tile_walk.h's walk_outward written out in place: the K-list of 3 K registers is live across the whole walk,
// and behind that function's boundary hipcc (ROCm 7.2) allocates 144 VGPRs at K = 16 where the loop in place takes 127 of the
// 128 that four waves per SIMD allow (tests/test_prepare_isa.py).
#pragma once
#include "prepare_math.h"
#include "tile_walk.h"

namespace usip_walk {

static_assert(usip_prep::TILE == WALK_TILE, "the K-list walk goes over tile_walk.h's tiles");

// R: the cloud -- R.n >= 1 rows, R.at(s) the original index of sorted position s < n (never outside [0, n)), R.row(j) the
// float4 of original row j.  SELF: a query is a neighbour of itself.  FOUR: four rows in flight with one test of the smallest
// of their distances in front; that test lets a row pass or fall by its neighbours' distances once one of them is NaN, so a
// cloud that may hold non-finite rows takes one row at a time.  tile, orig: two LDS slots of 256 rows; slots: 4 doubles.
// Workgroup b's live queries write their lists to idx[original index][K].  Returns the tiles walked.
template <int K, bool SELF, bool FOUR, class Rows>
__device__ __forceinline__ int nearest_rows(const Rows& R, int b, float4 (*tile)[WALK_TILE], int32_t (*orig)[WALK_TILE],
                                            double* slots, int32_t* __restrict__ idx)
{
    using usip_prep::sqdist;
    constexpr int TILE = WALK_TILE;
    const int l = threadIdx.x, n = R.n;
    const int q = b * TILE + l;                                        // position in the sorted order
    const bool live = q < n;
    const int me = R.at(live ? q : n - 1);
    const float4 p = R.row(me);
    const double xi = (double)p.x, yi = (double)p.y, zi = (double)p.z;
    const auto x_at = [&](int s) { return (double)R.row(R.at(s)).x; };
    const Tiles<decltype(x_at)> tiles(n, x_at);
    const double xlo = tiles.near_x(1, b), xhi = tiles.near_x(0, b);   // the x range of this workgroup's queries

    usip_prep::KList<K> list;
    list.clear();

    auto stage = [&](int slot, int t) {                                // tile t of the sorted order -> LDS
        const int s = t * TILE + l;
        const int j = R.at(s < n ? s : n - 1);
        tile[slot][l] = R.row(j);
        orig[slot][l] = j;
    };
    auto offer = [&](double d, int slot, int c) {
        if (d <= list.worst()) {                                       // rare after the first tiles
            const int32_t j = orig[slot][c];
            if ((SELF || j != me) && list.admits(d, j)) list.insert(d, j);
        }
    };
    auto walk = [&](int slot, int count) {
        int c = 0;
        if constexpr (FOUR) {
            for (; c + 4 <= count; c += 4) {                           // four rows in flight: the LDS latency overlaps
                const float4 o0 = tile[slot][c], o1 = tile[slot][c + 1], o2 = tile[slot][c + 2], o3 = tile[slot][c + 3];
                const double d0 = sqdist(xi, yi, zi, o0.x, o0.y, o0.z), d1 = sqdist(xi, yi, zi, o1.x, o1.y, o1.z);
                const double d2 = sqdist(xi, yi, zi, o2.x, o2.y, o2.z), d3 = sqdist(xi, yi, zi, o3.x, o3.y, o3.z);
                const double lo01 = d0 < d1 ? d0 : d1, lo23 = d2 < d3 ? d2 : d3;
                if ((lo01 < lo23 ? lo01 : lo23) <= list.worst()) {
                    offer(d0, slot, c);
                    offer(d1, slot, c + 1);
                    offer(d2, slot, c + 2);
                    offer(d3, slot, c + 3);
                }
            }
        }
        for (; c < count; ++c) {
            const float4 o = tile[slot][c];
            offer(sqdist(xi, yi, zi, o.x, o.y, o.z), slot, c);
        }
    };

    stage(0, b);
    __syncthreads();
    if (live) walk(0, tiles.rows(b));
    int left = b - 1, right = b + 1, seen = 1;
    while (true) {
        double unused = 0.0, bound = live ? list.worst() : -1.0;
        __syncthreads();                                               // the previous round's reads are done
        block_minmax<false, true>(unused, bound, slots);               // (also: every lane is done with the tiles)
        if (left >= 0) {
            const double gap = xlo - tiles.near_x(0, left);
            if (gap * gap > bound) left = -1;
        }
        if (right < tiles.tiles) {
            const double gap = tiles.near_x(1, right) - xhi;
            if (gap * gap > bound) right = tiles.tiles;
        }
        if (left < 0 && right >= tiles.tiles) break;                   // workgroup-uniform
        if (left >= 0) stage(0, left);
        if (right < tiles.tiles) stage(1, right);
        __syncthreads();
        if (left >= 0) {
            if (live) walk(0, tiles.rows(left));
            --left;
            ++seen;
        }
        if (right < tiles.tiles) {
            if (live) walk(1, tiles.rows(right));
            ++right;
            ++seen;
        }
    }
    if (live) {
#pragma unroll
        for (int k = 0; k < K; ++k) idx[(long long)me * K + k] = list.j[k];
    }
    return seen;
}

}  // namespace usip_walk
