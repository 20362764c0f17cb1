// usip_amd/csrc/ascending_walk.h -- the ASCENDING tile walk of the x-sorted baseline detectors and the kernel body around it:
// iss_saliency_kernel and iss_nms_kernel (csrc/iss.hip), harris_normals_kernel and harris_response_kernel (csrc/harris.hip),
// sift_dog_kernel<S> (csrc/sift.hip).  A workgroup of TILE lanes owns TILE consecutive queries of a frame sorted along x (the
// caller's permutation), one lane per query, what it gathers in registers; the frame is cut into tiles of TILE rows of that
// order, staged in LDS as 16-byte rows that every lane reads at the same address (broadcast reads), and the tiles that can hold
// a member are walked from low x to high x -- the order of the sums is part of these kernels' contracts, which is why they do
// not use tile_walk.h's outward walk.  The walk goes from the first tile whose largest x is within r of the workgroup's smallest
// query x to the last tile whose smallest x is within r of its largest.  A tile left out on the low side has gap =
// fl(xlo - xmax) >= r, so for every query x_i >= xlo and every point x_j <= xmax of it dx = fl(x_i - x_j) >= gap >= r (float64
// rounding is monotone), hence d2 = fl(fl(dx dx + dy dy) + dz dz) >= fl(dx dx) >= fl(r r) = r2: no member.  The high side
// likewise.  The result is the all-pairs answer, sums in the all-pairs order.  Device only.
//
// ascend(F, N, r, tile, visited, pass) is the whole kernel behind its arguments (iss_nms_kernel alone keeps its body in place
// over Frame and walk_tiles: csrc/iss.hip says why); a PASS is what one kernel does on the way:
//   ROWS                    rows of a tile in flight in the row loop (the LDS latency overlaps): 4, 2 or 1
//   Side, side(slot, c)     what row c of LDS slot `slot` holds beside its float4 (Plain: nothing)
//   stage(slot, l, j)       stages that for lane l's row, point j of the frame; returns the float4 row's fourth component
//   walks(live, me)         whether this lane offers rows at all; called once, before the walk (Plain: live)
//   offer(xi, yi, zi, o, s) one row to the lane's sums, which the pass holds
//   dead(q)                 the outputs of the dead slot q
//   write(me, xi, yi, zi)   the outputs of the live query at original index me
// Slots beyond count[b] get what dead() writes.  An entry of perm outside [0, count) reads point 0: a wrong permutation gives
// wrong values, never a wild read.
#pragma once
#include "common.h"
#include "bank.h"
#include "iss_math.h"

#define USIP_DEV __device__ __forceinline__

namespace usip_ascend {

using usip_iss::TILE;

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
        n = usip_iss::live_points(count, f, N);
    }
    __device__ __forceinline__ int at(int s) const { return usip_bank::safe_index(perm[s < n ? s : n - 1], n); }   // sorted -> original
    __device__ __forceinline__ float4 row(int j) const { return make_float4(x[j], y[j], z[j], 0.0f); }
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

// The walk.  stage(slot, t) copies tile t of the sorted order into LDS slot `slot`; first_x(slot) is the x of that slot's
// first row; walk(slot, rows) offers its rows to the lane in ascending order.  Returns the tiles walked.
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

// The parts of a pass that only some kernels have
struct Plain {
    struct Side {};
    USIP_DEV Side side(int, int) const { return {}; }
    USIP_DEV float stage(int, int, int) const { return 0.0f; }
    USIP_DEV bool walks(bool live, int) const { return live; }
};

// The kernel: grid = (tiles of a frame, B), TILE lanes, tile = two LDS slots of TILE rows.  visited (or nullptr): the tiles
// each workgroup walked, i32 [B][gridDim.x].  No atomics, no float reduction across lanes.
template <class Pass>
__device__ __forceinline__ void ascend(const Frame& F, int N, double r, float4 (*tile)[TILE], int32_t* visited, Pass& pass)
{
    const int l = threadIdx.x, w = blockIdx.x, f = blockIdx.y;
    const int q = w * TILE + l;                                        // position in the sorted order
    const auto report = [&](int seen) {
        if (visited && l == 0) visited[(long long)f * gridDim.x + w] = seen;
    };
    if (q >= F.n && q < N) pass.dead(q);                               // a dead slot: q itself (the live ones are 0 .. n-1)
    if (w * TILE >= F.n) return report(0);                             // workgroup-uniform: no query here
    const bool live = q < F.n;
    const int me = F.at(q);
    const double xi = (double)F.x[me], yi = (double)F.y[me], zi = (double)F.z[me];
    const int seen = walk_tiles(
        F, w, r, pass.walks(live, me),
        [&](int slot, int t) {
            const int j = F.at(t * TILE + l);
            tile[slot][l] = make_float4(F.x[j], F.y[j], F.z[j], pass.stage(slot, l, j));
        },
        [&](int slot) { return (double)tile[slot][0].x; },
        [&](int slot, int rows) {
            constexpr int R = Pass::ROWS;
            int c = 0;
            if constexpr (R > 1) {
                for (; c + R <= rows; c += R) {
                    float4 o[R];
                    typename Pass::Side s[R];
#pragma unroll
                    for (int k = 0; k < R; ++k) o[k] = tile[slot][c + k];
#pragma unroll
                    for (int k = 0; k < R; ++k) s[k] = pass.side(slot, c + k);
#pragma unroll
                    for (int k = 0; k < R; ++k) pass.offer(xi, yi, zi, o[k], s[k]);
                }
            }
            for (; c < rows; ++c) pass.offer(xi, yi, zi, tile[slot][c], pass.side(slot, c));
        });
    if (live) pass.write(me, xi, yi, zi);
    report(seen);
}

}  // namespace usip_ascend
