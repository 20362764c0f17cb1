// usip_amd/csrc/cell_grid.hip -- a uniform cell grid over a cloud, and the step's two point searches through it.
//
// ball_query_coords_kernel and nearest_kernel compare every node / keypoint with every point of its cloud: 134 M pair
// tests each in the detector step, for balls that hold ~20 points.  Both answers are sets -- "the K smallest indices
// with s <= T", "the minimum, then the lowest index" -- and do not depend on the order of evaluation, so testing only
// the points of the cells around the query gives the same bits:
//   cell_grid_build_kernel   bounding box, grid header, counting sort of the points by cell (cell_start, and the
//                            points as (x, y, z, index) in cell order: a cell is one contiguous read).  BUILD_S
//                            workgroups per cloud, each sorting the points of its own eighth of the cells
//   ball_query_grid_kernel   one wave per node row: the 3 x 3 x 3 cells around the node's cell
//   nearest_grid_kernel      one wave per four queries, one after the other: the 27 cells around the query's cell,
//                            then blocks growing ring by ring until no unscanned cell can hold the answer
// A row the grid cannot answer (unusable cloud, too many candidates, ring cap) runs the index-order scan of
// pair_scan.h inside the same launch: nothing is decided on the host from device data.  The cell arithmetic and the
// argument for it are in cell_grid.h.
#include "cell_grid.h"
#include "pair_scan.h"
#include <cstring>

namespace {

constexpr int BUILD_T = 1024;
constexpr int BUILD_U = 8;                 // points per thread in flight: one exposed load latency per 8192 points, not per 1024
constexpr int BUILD_S = 8;                 // workgroups per cloud.  The sort is bound by LDS atomics (about one per clock and
                                           // CU: one workgroup per cloud took 26 us for 16384 points); every workgroup reads
                                           // the whole cloud but counts and places only the points of its own range of cells
constexpr int BUILD_RANGE = USIP_CELL_CAP / BUILD_S + 1;
constexpr int BUILD_MAX_N = 1 << 20;       // every workgroup reads the whole cloud; beyond this the searches scan
constexpr int BQ_CAND = 512;               // longest grid scan of a ball-query row = length of its hit list
constexpr int NEAREST_RINGS = 3;           // blocks of 3^3, 5^3, 7^3 cells (at most 49 runs: one per lane)
constexpr int NEAREST_CAND = 1024;         // largest block of candidates a query reads through the grid
constexpr int NEAREST_R = 4;               // queries per wave, as nearest_kernel

__device__ __forceinline__ bool finite_f32(float v) { return fabsf(v) <= 3.4028234664e38f; }    // false for NaN

__global__ __launch_bounds__(BUILD_T) void cell_grid_build_kernel(
    const float* __restrict__ x, float edge_req, int max_block, int32_t* __restrict__ hdr,
    int32_t* __restrict__ cell_start, float4* __restrict__ pts, int N)
{
    __shared__ int cnt[BUILD_RANGE];                      // counters of this workgroup's cells, then their cursors
    __shared__ float s_lo[3][BUILD_T / 64], s_hi[3][BUILD_T / 64];
    __shared__ int s_bad[BUILD_T / 64], s_wsum[BUILD_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, part = blockIdx.y;
    const float* xb = x + (long long)b * 3 * N;
    int32_t* h = hdr + (long long)b * USIP_CELL_HDR_WORDS;
    int32_t* cs = cell_start + (long long)b * (USIP_CELL_CAP + 1);
    float4* pb = pts + (long long)b * N;

    // bounding box of the points; any non-finite coordinate makes the cloud unusable
    float lo[3], hi[3];
    int bad = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) { lo[d] = __builtin_inff(); hi[d] = -__builtin_inff(); }
    if (N <= BUILD_MAX_N)
        for (int i0 = tid; i0 < N; i0 += BUILD_T * BUILD_U) {
            float v[BUILD_U][3];
#pragma unroll
            for (int u = 0; u < BUILD_U; ++u) {            // the tail repeats the cloud's last point: same box
                const int i = min(i0 + u * BUILD_T, N - 1);
#pragma unroll
                for (int d = 0; d < 3; ++d) v[u][d] = xb[(long long)d * N + i];
            }
#pragma unroll
            for (int u = 0; u < BUILD_U; ++u)
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    bad |= finite_f32(v[u][d]) ? 0 : 1;
                    lo[d] = fminf(lo[d], v[u][d]); hi[d] = fmaxf(hi[d], v[u][d]);
                }
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = fminf(lo[d], __shfl_xor(lo[d], off)); hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], off));
        }
        bad |= __shfl_xor(bad, off);
    }
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { s_lo[d][wave] = lo[d]; s_hi[d][wave] = hi[d]; }
        s_bad[wave] = bad;
    }
    __syncthreads();
    for (int w = 0; w < BUILD_T / 64; ++w) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { lo[d] = fminf(lo[d], s_lo[d][w]); hi[d] = fmaxf(hi[d], s_hi[d][w]); }
        bad |= s_bad[w];
    }

    // the header, by every thread alike (the same operations on the same values).  The edge only ever grows from
    // the requested one: by 2 while the grid is far too fine, then by 1/8 until its cells fit the counters.
    bool usable = !bad && N >= 1 && N <= BUILD_MAX_N && finite_f32(edge_req) && edge_req >= USIP_CELL_MIN_EDGE &&
                  finite_f32(hi[0] - lo[0]) && finite_f32(hi[1] - lo[1]) && finite_f32(hi[2] - lo[2]);
    usip_cell_hdr g;
    g.edge = edge_req; g.inv = 0.f; g.n[0] = g.n[1] = g.n[2] = 1;
#pragma unroll
    for (int d = 0; d < 3; ++d) g.o[d] = lo[d];
    if (usable) {
        bool fits = false;
        for (int it = 0; it < 400 && !fits; ++it) {
            g.inv = 1.0f / g.edge;
            float cells = 1.f;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                g.n[d] = usip_cell_coord(hi[d], lo[d], g.inv, 1 << 24) + 1;      // n = c(vmax) + 1, cell_grid.h (1)
                cells *= (float)g.n[d];
            }
            fits = cells <= (float)USIP_CELL_CAP;
            if (!fits) g.edge *= cells > 8.f * USIP_CELL_CAP ? 2.0f : 1.125f;
            if (!finite_f32(g.edge)) break;
        }
        usable = fits;
        // A dense cloud: the block of 3 x 3 x 3 cells (fewer at a grid one or two cells thin) around a query holds on
        // average more points than the caller's searches would take through the grid (for the ball query the row rule
        // cand^2 <= N K of ball_query_grid_kernel, which the caller states as max_block = sqrt(N K)).  Every row would
        // scan anyway: the cloud is left unsorted and unusable, and the build ends after its bounding-box pass.
        if (fits && max_block > 0) {
            const float block = (float)(min(g.n[0], 3) * min(g.n[1], 3) * min(g.n[2], 3));
            usable = block * (float)N <= (float)max_block * (float)(g.n[0] * g.n[1] * g.n[2]);
        }
    }
    if (tid == 0 && part == 0) {
        h[USIP_CELL_OX] = __float_as_int(g.o[0]); h[USIP_CELL_OY] = __float_as_int(g.o[1]);
        h[USIP_CELL_OZ] = __float_as_int(g.o[2]);
        h[USIP_CELL_EDGE] = __float_as_int(g.edge); h[USIP_CELL_INV] = __float_as_int(g.inv);
        h[USIP_CELL_NX] = g.n[0]; h[USIP_CELL_NY] = g.n[1]; h[USIP_CELL_NZ] = g.n[2];
        h[USIP_CELL_USABLE] = usable ? 1 : 0;
    }
    if (!usable) return;                                   // every workgroup of the cloud alike

    // counting sort by cell: this workgroup's cells are [r0, r1); `below` counts the points of the cells before them
    const int cells = g.n[0] * g.n[1] * g.n[2];
    const int r0 = (int)((long long)cells * part / BUILD_S), r1 = (int)((long long)cells * (part + 1) / BUILD_S);
    for (int c = tid; c < r1 - r0; c += BUILD_T) cnt[c] = 0;
    int below = 0;
    __syncthreads();
    for (int i0 = tid; i0 < N; i0 += BUILD_T * BUILD_U) {
        float v[BUILD_U][3];
#pragma unroll
        for (int u = 0; u < BUILD_U; ++u) {
            const int i = min(i0 + u * BUILD_T, N - 1);
#pragma unroll
            for (int d = 0; d < 3; ++d) v[u][d] = xb[(long long)d * N + i];
        }
#pragma unroll
        for (int u = 0; u < BUILD_U; ++u)
            if (i0 + u * BUILD_T < N) {
                const int c = usip_cell_id(g, usip_cell_coord(v[u][0], g.o[0], g.inv, g.n[0]),
                                           usip_cell_coord(v[u][1], g.o[1], g.inv, g.n[1]),
                                           usip_cell_coord(v[u][2], g.o[2], g.inv, g.n[2]));
                if (c >= r0 && c < r1) atomicAdd(&cnt[c - r0], 1);
                below += c < r0 ? 1 : 0;
            }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) below += __shfl_xor(below, off);
    __syncthreads();                                       // (s_bad is free again: every thread has read it)
    if (lane == 0) s_bad[wave] = below;
    // exclusive prefix over the cells: a thread owns `per` consecutive cells of the range
    const int per = (r1 - r0 + BUILD_T - 1) / BUILD_T;
    const int c0 = min(tid * per, r1 - r0), c1 = min(c0 + per, r1 - r0);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += cnt[c];
    int incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int run = incl - sum;
    for (int w = 0; w < wave; ++w) run += s_wsum[w];
    for (int w = 0; w < BUILD_T / 64; ++w) run += s_bad[w];
    for (int c = c0; c < c1; ++c) {
        const int v = cnt[c];
        cnt[c] = run;                                      // from here on the cell's write cursor
        cs[r0 + c] = run;
        run += v;
    }
    if (part == BUILD_S - 1 && tid == 0) cs[cells] = N;    // every point is finite and lands in a cell
    __syncthreads();
    // the order inside a cell is whatever the cursors give; both searches are independent of it
    for (int i0 = tid; i0 < N; i0 += BUILD_T * BUILD_U) {
        float v[BUILD_U][3];
#pragma unroll
        for (int u = 0; u < BUILD_U; ++u) {
            const int i = min(i0 + u * BUILD_T, N - 1);
#pragma unroll
            for (int d = 0; d < 3; ++d) v[u][d] = xb[(long long)d * N + i];
        }
#pragma unroll
        for (int u = 0; u < BUILD_U; ++u) {
            const int i = i0 + u * BUILD_T;
            const int c = usip_cell_id(g, usip_cell_coord(v[u][0], g.o[0], g.inv, g.n[0]),
                                       usip_cell_coord(v[u][1], g.o[1], g.inv, g.n[1]),
                                       usip_cell_coord(v[u][2], g.o[2], g.inv, g.n[2]));
            if (i < N && c >= r0 && c < r1) {
                const int pos = atomicAdd(&cnt[c - r0], 1);
                pb[pos] = make_float4(v[u][0], v[u][1], v[u][2], __int_as_float(i));
            }
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void ball_query_grid_kernel(
    const float* __restrict__ node, const float* __restrict__ x, const int32_t* __restrict__ hdr,
    const int32_t* __restrict__ cell_start, const float4* __restrict__ pts, int32_t* __restrict__ out,
    uint8_t* __restrict__ route, float T, float min_edge, int K, int M, int N)
{
    extern __shared__ __attribute__((aligned(16))) int smem[];      // [4 waves][K list | BQ_CAND hits]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int m = blockIdx.x * 4 + wave;
    int* list = smem + wave * (K + BQ_CAND);
    int* hits = list + K;
    const float* xb = x + (long long)b * 3 * N;
    const float* nb = node + (long long)b * 3 * M;

    int count[1] = {K};
    if (m < M) {
        const usip_cell_hdr g = usip_cell_load_hdr(hdr + (long long)b * USIP_CELL_HDR_WORDS);
        bool grid = false;
        // the grid serves this radius only if its cells are at least radius * USIP_CELL_MIN_EDGE_FACTOR wide (cell_grid.h (3));
        // false for an infinite or NaN radius
        if (g.usable && g.edge >= min_edge) {
            const float ax = nb[m], ay = nb[M + m], az = nb[2 * M + m];
            const int c[3] = {usip_cell_coord(ax, g.o[0], g.inv, g.n[0]), usip_cell_coord(ay, g.o[1], g.inv, g.n[1]),
                              usip_cell_coord(az, g.o[2], g.inv, g.n[2])};
            int lo[3], hi[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) { lo[d] = max(c[d] - 1, 0); hi[d] = min(c[d] + 1, g.n[d] - 1); }
            int start, off, nruns;
            const int cand = usip_cell_block_runs(g, cell_start + (long long)b * (USIP_CELL_CAP + 1), lo, hi, lane,
                                                  start, off, nruns);
            // The index-order scan ends after K hits.  All `cand` candidates being hits, it would still read
            // N * K / cand points: with cand^2 <= N * K the grid tests no more points than the shortest scan this row
            // can have.  Beyond that (dense clouds) the scan's early exit is the better route.
            grid = cand <= BQ_CAND && (long long)cand * cand <= (long long)N * K;
            if (grid) {
                const float4* pb = pts + (long long)b * N;
                int u = 0;
                for (int t0 = 0; t0 < cand; t0 += 64) {
                    const int t = t0 + lane;
                    const float4 p = pb[usip_cell_candidate(min(t, cand - 1), start, off, nruns)];
                    const bool hit = t < cand && usip_sqdist(ax, ay, az, p.x, p.y, p.z) <= T;
                    const unsigned long long mask = __ballot(hit);
                    if (hit) hits[u + usip_mbcnt(mask)] = __float_as_int(p.w);      // u <= t0: never past BQ_CAND
                    u += __popcll(mask);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                // indices are distinct: the rank of a hit among the hits is its place in the ascending row
                for (int i = lane; i < u; i += 64) {
                    const int v = hits[i];
                    int rank = 0;
                    for (int j = 0; j < u; ++j) rank += hits[j] < v ? 1 : 0;
                    if (rank < K) list[rank] = v;
                }
                count[0] = u;
            }
        }
        if (!grid) usip_ball_scan_rows<VEC, 1>(nb, xb, list, count, T, K, M, N, m, lane);
        if (route && lane == 0) route[(long long)b * M + m] = grid ? USIP_ROUTE_GRID : USIP_ROUTE_SCAN;
    }
    __syncthreads();
    usip_ball_write_rows<1>(list, count, out + ((long long)b * M + m) * K, K, M, m, lane);
}

__global__ __launch_bounds__(256) void nearest_grid_kernel(
    const float* __restrict__ a, const float* __restrict__ x, const int32_t* __restrict__ hdr,
    const int32_t* __restrict__ cell_start, const float4* __restrict__ pts, float* __restrict__ min_d,
    int32_t* __restrict__ arg, uint8_t* __restrict__ route, int Ma, int N)
{
    constexpr int R = NEAREST_R;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bi = blockIdx.y;
    const int i0 = (blockIdx.x * 4 + wave) * R;
    if (i0 >= Ma) return;
    const float* ab = a + (long long)bi * 3 * Ma;
    const float* xb = x + (long long)bi * 3 * N;
    const float4* pb = pts + (long long)bi * N;
    const int32_t* cs = cell_start + (long long)bi * (USIP_CELL_CAP + 1);
    const usip_cell_hdr g = usip_cell_load_hdr(hdr + (long long)bi * USIP_CELL_HDR_WORDS);

    unsigned scan = 0;                                     // bit r: query i0 + r goes to the index-order scan
#pragma unroll 1
    for (int r = 0; r < R && i0 + r < Ma; ++r) {
        const int i = i0 + r;
        const float q[3] = {ab[i], ab[Ma + i], ab[2 * Ma + i]};
        bool found = false;
        if (g.usable) {
            int c[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) c[d] = usip_cell_coord(q[d], g.o[d], g.inv, g.n[d]);
            bool dense = false;
#pragma unroll 1
            for (int k = 1; k <= NEAREST_RINGS && !found && !dense; ++k) {
                int lo[3], hi[3];
                float gap = __builtin_inff();
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    lo[d] = max(c[d] - k, 0); hi[d] = min(c[d] + k, g.n[d] - 1);
                    const float gd = usip_cell_gap(q[d], g.o[d], g.edge, lo[d], hi[d], g.n[d]);
                    gap = gd < gap ? gd : gap;
                }
                int start, off, nruns;
                const int cand = usip_cell_block_runs(g, cs, lo, hi, lane, start, off, nruns);
                // A candidate through the grid costs several times a pair of the index-order scan (its position is looked
                // up, its load is not streamed, the wave's other queries do not share it): a block of more than
                // NEAREST_CAND candidates is left to the scan.  The count is known before any candidate is read, and the
                // search starts with the 27 cells (the query's own cell alone settles too few queries to be worth a
                // pass of its own): a query that ends in the scan has read at most the blocks below the cap.
                dense = cand > NEAREST_CAND;
                if (dense) break;
                // per lane the two smallest squared distances of the block, the smallest with its index, lower index
                // first on equal squares (NaN never wins)
                float s0 = __builtin_inff(), s1 = __builtin_inff();
                int j0 = 0x7fffffff;
                for (int t0 = 0; t0 < cand; t0 += 64) {
                    const int t = t0 + lane;
                    const float4 p = pb[usip_cell_candidate(min(t, cand - 1), start, off, nruns)];
                    const float s = t < cand ? usip_sqdist(q[0], q[1], q[2], p.x, p.y, p.z) : __builtin_inff();
                    const int j = __float_as_int(p.w);
                    const bool first = s < s0 || (s == s0 && j < j0);
                    s1 = first ? s0 : (s < s1 ? s : s1);
                    j0 = first ? j : j0;
                    s0 = first ? s : s0;
                }
                float smin = s0;
#pragma unroll
                for (int o2 = 32; o2 > 0; o2 >>= 1) smin = fminf(smin, __shfl_xor(smin, o2));
                // Candidates that can be the answer have s <= thr (pair_scan.h).  An unscanned point is at least `gap`
                // away along some axis, so its s is at least gap^2 (1 - 2^-21); the factor below is 1 - 2^-20 and the
                // product is rounded twice by 2^-24.  When in doubt, another ring.
                const float thr = smin * 1.00000095367431640625f;          // 1 + 2^-20
                const float bound = gap > 0.f ? gap * gap * 0.99999904632568359375f : 0.f;
                found = thr < bound;                                       // false for an empty block (thr = inf)
                if (found) {
                    // Each lane's smallest is its only candidate within thr unless its second smallest is within thr too;
                    // then (rare: two points within 2^-20 of the minimum in one lane) the block is read again.
                    float bd = s0 <= thr ? sqrtf(s0) : __builtin_inff();
                    int bj = s0 <= thr ? j0 : 0x7fffffff;
                    if (__any(s1 <= thr)) {
                        bd = __builtin_inff(); bj = 0x7fffffff;
                        for (int t0 = 0; t0 < cand; t0 += 64) {
                            const int t = t0 + lane;
                            const float4 p = pb[usip_cell_candidate(min(t, cand - 1), start, off, nruns)];
                            const float s = usip_sqdist(q[0], q[1], q[2], p.x, p.y, p.z);
                            if (t < cand && s <= thr) {
                                const float d = sqrtf(s);
                                const int j = __float_as_int(p.w);
                                if (d < bd || (d == bd && j < bj)) { bd = d; bj = j; }
                            }
                        }
                    }
#pragma unroll
                    for (int o2 = 32; o2 > 0; o2 >>= 1) {
                        const float od = __shfl_xor(bd, o2);
                        const int oj = __shfl_xor(bj, o2);
                        if (od < bd || (od == bd && oj < bj)) { bd = od; bj = oj; }
                    }
                    if (lane == 0) {
                        min_d[(long long)bi * Ma + i] = bd;
                        arg[(long long)bi * Ma + i] = bj;
                    }
                }
            }
        }
        if (!found) scan |= 1u << r;
        if (route && lane == 0) route[(long long)bi * Ma + i] = found ? USIP_ROUTE_GRID : USIP_ROUTE_SCAN;
    }
    if (scan) {                                            // wave-uniform
        float d[R];
        int j[R];
        usip_nearest_scan<R>(ab, xb, Ma, N, 0, N, i0, lane, d, j);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (lane == 0 && i0 + r < Ma && (scan >> r & 1u)) {
                min_d[(long long)bi * Ma + i0 + r] = d[r];
                arg[(long long)bi * Ma + i0 + r] = j[r] == 0x7fffffff ? 0 : j[r];      // all-NaN row
            }
        }
    }
}

}  // namespace

extern "C" int usip_cell_grid_cap(void) { return USIP_CELL_CAP; }

extern "C" float usip_cell_grid_edge_factor(void) { return USIP_CELL_EDGE_FACTOR; }

extern "C" int usip_cell_grid_hdr_word(const char* name)
{
    static const struct { const char* name; int word; } words[] = {
        {"words", USIP_CELL_HDR_WORDS}, {"ox", USIP_CELL_OX}, {"oy", USIP_CELL_OY}, {"oz", USIP_CELL_OZ},
        {"edge", USIP_CELL_EDGE}, {"inv", USIP_CELL_INV}, {"nx", USIP_CELL_NX}, {"ny", USIP_CELL_NY},
        {"nz", USIP_CELL_NZ}, {"usable", USIP_CELL_USABLE}};
    for (const auto& w : words)
        if (name && strcmp(name, w.name) == 0) return w.word;
    return USIP_EINVAL;
}

extern "C" int usip_cell_grid_build_f32(const float* x, float edge, int max_block, int32_t* hdr, int32_t* cell_start,
                                        float* pts, int B, int N, void* stream)
{
    if (B < 0 || N < 0 || max_block < 0) return USIP_EINVAL;
    if (B == 0) return USIP_OK;
    if (!hdr || !cell_start || (N > 0 && (!x || !pts)) || B > 65535) return USIP_EINVAL;
    if (reinterpret_cast<uintptr_t>(pts) & 15u) return USIP_EINVAL;
    USIP_LAUNCH(cell_grid_build_kernel, dim3(B, BUILD_S), dim3(BUILD_T), 0, (hipStream_t)stream, x, edge, max_block, hdr, cell_start, reinterpret_cast<float4*>(pts), N);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_ball_query_grid_f32(const float* node, const float* x, const int32_t* hdr,
                                        const int32_t* cell_start, const float* pts, int32_t* out_idx, uint8_t* route,
                                        float radius, int K, int B, int M, int N, void* stream)
{
    if (B < 0 || M < 0 || N < 0 || K < 0) return USIP_EINVAL;
    if ((long long)B * M == 0 || K == 0) return USIP_OK;
    if (!node || !x || !out_idx || !hdr || !cell_start || !pts) return USIP_EINVAL;
    if (K > 1024 || B > 65535 || (reinterpret_cast<uintptr_t>(pts) & 15u)) return USIP_EINVAL;
    const float T = usip_sqrt_threshold(radius);
    const float min_edge = radius * USIP_CELL_MIN_EDGE_FACTOR;      // cell_grid.h (3): what the argument needs, below what is asked for
    const bool vec = (N >= 4) && (N % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15u) == 0);
    const dim3 grid(usip_ceil_div(M, 4), B), block(256);
    const size_t lds = (size_t)4 * (K + BQ_CAND) * sizeof(int);
    const float4* p4 = reinterpret_cast<const float4*>(pts);
    if (vec)
        USIP_LAUNCH((ball_query_grid_kernel<true>), grid, block, lds, (hipStream_t)stream, node, x, hdr, cell_start, p4,
                    out_idx, route, T, min_edge, K, M, N);
    else
        USIP_LAUNCH((ball_query_grid_kernel<false>), grid, block, lds, (hipStream_t)stream, node, x, hdr, cell_start, p4,
                    out_idx, route, T, min_edge, K, M, N);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_nearest_grid_f32(const float* a, const float* x, const int32_t* hdr, const int32_t* cell_start,
                                     const float* pts, float* min_d, int32_t* arg, uint8_t* route, int B, int Ma, int N,
                                     void* stream)
{
    if (B < 0 || Ma < 0 || N < 1) return USIP_EINVAL;
    if ((long long)B * Ma == 0) return USIP_OK;
    if (!a || !x || !hdr || !cell_start || !pts || !min_d || !arg || B > 65535) return USIP_EINVAL;
    if (reinterpret_cast<uintptr_t>(pts) & 15u) return USIP_EINVAL;
    USIP_LAUNCH(nearest_grid_kernel, dim3(usip_ceil_div(Ma, 4 * NEAREST_R), B), dim3(256), 0, (hipStream_t)stream,
                a, x, hdr, cell_start, reinterpret_cast<const float4*>(pts), min_d, arg, route, Ma, N);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
