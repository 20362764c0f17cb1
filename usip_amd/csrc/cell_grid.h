// usip_amd/csrc/cell_grid.h -- the cell arithmetic of the uniform grid (csrc/cell_grid.hip): one copy for the kernel
// that sorts a cloud into cells and for the two searches that read it.
//
// A cloud's grid is its header (USIP_CELL_* words, include/usip_hip.h): origin o = the per-axis minimum of the points,
// edge e, inv = 1 / e as the build rounded it, and the dimensions.  The cell coordinate of v along one axis is
//
//     c(v) = clamp(floor(fl(fl(v - o) * inv)), 0, n - 1),          n = c(vmax) + 1 with the same function.
//
// Facts the searches rest on:
//   (1) c is monotone in v: a rounded subtraction of a constant, a rounded product with a positive constant, floor
//       and clamp are each monotone.  Hence c(vmin) = 0 and c(vmax) = n - 1, and the clamp changes nothing for a point
//       of the cloud itself.
//   (2) u(v) = fl(fl(v - o) * inv) = (v - o) / e * (1 + eps) with |eps| < 2^-22: three roundings of 2^-24 each (the
//       difference, inv = fl(1 / e), the product).  Every n is at most USIP_CELL_CAP < 2^14, so for cloud points a <= b
//       u(b) - u(a) <= (b - a) / e + 2 * 2^-22 * 2^14 = (b - a) / e + 2^-7.
//   (3) The ball query takes a grid with e >= radius * USIP_CELL_MIN_EDGE_FACTOR = radius * (1 + 2^-6); coarsening only
//       grows e.  Callers ask for radius * USIP_CELL_EDGE_FACTOR = radius * (1 + 2^-5), so that a product rounded in
//       another precision on their side still clears the kernel's own float product by far.
//       A hit of the ball query has s <= T, so every |a_d - b_d| <= radius * (1 + 2^-22) (the three terms of s are
//       non-negative and each rounding is relative; the build refuses edges below 2^-50 so that no square of a
//       difference that matters underflows).  Then (b - a) / e <= (1 + 2^-22) / (1 + 2^-6) < 0.9847, with (2)
//       u(b) - u(a) < 0.993 < 1, and floor(u(b)) <= floor(u(a) + 1): two points no farther apart than the radius never
//       land more than one cell apart, whatever the roundings did.
//   (4) A node outside the box is clamped.  Above the box: c(node) = n - 1 >= c(p) for every point p, and a point p
//       within the radius of the node is within the radius of vmax along that axis, so c(p) >= c(vmax) - 1 = n - 2 by
//       (3).  Below the box the same with vmin and cell 0.  A NaN node coordinate goes to cell 0; it has no hits.
//   (5) Bounds for the nearest search: a point with c(v) >= m has u(v) >= m, so v - o >= m * e * (1 - 2^-22); a point
//       with c(v) < m has v - o < m * e * (1 + 2^-22).  usip_cell_gap() turns that into a distance no unscanned point
//       can undercut.
#pragma once
#include "common.h"

#define USIP_CELL_EDGE_FACTOR 1.03125f          /* 1 + 2^-5: what callers ask for, see (3) */
#define USIP_CELL_MIN_EDGE_FACTOR 1.015625f     /* 1 + 2^-6: what the ball query insists on */
#define USIP_CELL_MIN_EDGE 0x1p-50f

struct usip_cell_hdr {
    float o[3], edge, inv;
    int n[3], usable;
};

__device__ __forceinline__ usip_cell_hdr usip_cell_load_hdr(const int32_t* __restrict__ h)
{
    usip_cell_hdr g;
    g.o[0] = __int_as_float(h[USIP_CELL_OX]); g.o[1] = __int_as_float(h[USIP_CELL_OY]);
    g.o[2] = __int_as_float(h[USIP_CELL_OZ]);
    g.edge = __int_as_float(h[USIP_CELL_EDGE]); g.inv = __int_as_float(h[USIP_CELL_INV]);
    g.n[0] = h[USIP_CELL_NX]; g.n[1] = h[USIP_CELL_NY]; g.n[2] = h[USIP_CELL_NZ];
    g.usable = h[USIP_CELL_USABLE];
    return g;
}

// c(v) above; n >= 1.  fmaxf drops a NaN, so the conversion never sees one.
__device__ __forceinline__ int usip_cell_coord(float v, float o, float inv, int n)
{
    const float u = floorf((v - o) * inv);
    return (int)fminf(fmaxf(u, 0.0f), (float)(n - 1));
}

// Cells are numbered x fastest: the cells lo_x .. hi_x of one (y, z) are one contiguous run of the sorted points.
__device__ __forceinline__ int usip_cell_id(const usip_cell_hdr& g, int cx, int cy, int cz)
{
    return (cz * g.n[1] + cy) * g.n[0] + cx;
}

// The block of cells [lo, hi] (inside the grid) as runs of sorted points, one run per (y, z), held by the lanes:
// lane r < nruns has its run's first sorted position in `start` and the number of candidates of the runs before it in
// `off`.  Returns the block's candidate count.  nruns <= 64.
__device__ __forceinline__ int usip_cell_block_runs(const usip_cell_hdr& g, const int32_t* __restrict__ cs,
                                                    const int (&lo)[3], const int (&hi)[3], int lane,
                                                    int& start, int& off, int& nruns)
{
    const int ny = hi[1] - lo[1] + 1;
    nruns = ny * (hi[2] - lo[2] + 1);
    int len = 0;
    start = 0;
    if (lane < nruns) {
        const int base = usip_cell_id(g, 0, lo[1] + lane % ny, lo[2] + lane / ny);
        start = cs[base + lo[0]];
        len = cs[base + hi[0] + 1] - start;
    }
    int incl = len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    off = incl - len;
    return __shfl(incl, 63);
}

// Sorted position of the block's candidate t (t < the block's count; every lane of the wave calls this together):
// the run r with off[r] <= t < off[r + 1], found by bisection over the lanes' `off`.
__device__ __forceinline__ int usip_cell_candidate(int t, int start, int off, int nruns)
{
    int a = 0, b = nruns - 1;
#pragma unroll 1
    for (int it = 0; (1 << it) < nruns; ++it) {          // wave-uniform trip count: every lane runs all steps (shuffles)
        const int mid = (a + b + 1) >> 1;
        const bool ge = __shfl(off, mid) <= t;
        const bool open = a < b;
        a = (open && ge) ? mid : a;
        b = (open && !ge) ? mid - 1 : b;
    }
    return __shfl(start, a) + (t - __shfl(off, a));
}

// Lower bound on |v - q| along one axis for every cloud point v outside the scanned cells [lo, hi] of that axis
// ((5) above), made smaller by 2^-20 of the magnitudes involved -- far more than the three roundings of the
// expression and the 2^-22 of (5).  +inf where the block reaches the grid's border; may be <= 0 (never stops a search).
__device__ __forceinline__ float usip_cell_gap(float q, float o, float edge, int lo, int hi, int n)
{
    float gap = __builtin_inff();
    if (hi < n - 1) {
        const float w = (float)(hi + 1) * edge;
        gap = ((w + o) - q) - 0x1p-20f * (fabsf(w) + fabsf(o) + fabsf(q));
    }
    if (lo > 0) {
        const float w = (float)lo * edge;
        const float down = (q - (w + o)) - 0x1p-20f * (fabsf(w) + fabsf(o) + fabsf(q));
        gap = down < gap ? down : gap;                   // (a NaN gap never stops a search: its query has no finite distance)
    }
    return gap;
}
