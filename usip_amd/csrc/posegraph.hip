// usip_amd/csrc/posegraph.hip -- the dense information matrix of aligned fragment pairs and the robust pose-graph optimiser
// that prunes loop closures, on the device.  csrc/posegraph_math.h has the arithmetic, which the host twin
// (csrc/posegraph_cpu.cpp) shares; include/usip_hip.h (f-14) is the contract.  No launch synchronises, no floating-point
// atomics, every index read from memory is checked or clamped before use.
//
//   icp_information_kernel   one workgroup per pair: lane l adds the terms of its rows l, l + 256, ... that lie within the
//                            radius, at the fragment-1 row the nearest pass named; registration_math.h's tree; lane 0 fills
//                            the 6 x 6.
//   posegraph_kernel         one workgroup of 256 lanes per scene, both stages and every iteration inside: the edge pass (a
//                            lane per edge: residual, weight, the edge's blocks), the assembly (a lane per entry, every
//                            sum over the node's incidence list in ascending edge index), the Cholesky factorisation of
//                            the 6 (n - 1)-square system in the workspace (column k of the factor contiguous, so the lanes
//                            of a column read consecutive addresses; lane l owns rows l, l + 256, l + 512 and keeps their
//                            running values in registers), the two substitutions with the solution in LDS, the update.
//                            __syncthreads() orders the workgroup's global writes between the phases.
#include "common.h"
#include "bank.h"
#include "posegraph_math.h"

using namespace usip_pg;
using usip_frag::info_fill;
using usip_frag::info_terms;
using usip_frag::radius_sq_hi;
using usip_frag::within;
using usip_bank::bank_ok;
using usip_bank::fragment_range;
using usip_bank::Range;
using usip_reg::tree_sum;

namespace {

__global__ __launch_bounds__(LANES) void icp_information_kernel(const float* __restrict__ rows, int row_len,
                                                                const int64_t* __restrict__ offsets, int num_frags,
                                                                long long total, const int32_t* __restrict__ frag1,
                                                                const int32_t* __restrict__ frag2,
                                                                const int32_t* __restrict__ idx, const double* __restrict__ d2,
                                                                const uint8_t* __restrict__ mask, double radius, double r2hi,
                                                                int Lmax, double* __restrict__ info, int32_t* __restrict__ count)
{
    __shared__ double part[LANES][10];
    const int p = blockIdx.x, l = threadIdx.x;
    const Range r1 = fragment_range(offsets, num_frags, total, frag1[p], Lmax);
    const Range r2 = fragment_range(offsets, num_frags, total, frag2[p], Lmax);
    const bool live = !(mask && mask[p] == 0) && r1.n >= 1;            // workgroup-uniform
    const int n2 = live ? r2.n : 0;
    const float* rows1 = rows + r1.first * row_len;
    double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int mine = 0;
    for (int i = l; i < n2; i += LANES)
        if (within(d2[(long long)p * Lmax + i], radius, r2hi)) {
            const float* a = rows1 + (long long)clamp_index(idx[(long long)p * Lmax + i], r1.n) * row_len;
            double t[9];
            info_terms((double)a[0], (double)a[1], (double)a[2], t);
#pragma unroll
            for (int k = 0; k < 9; ++k) s[k] += t[k];
            ++mine;
        }
#pragma unroll
    for (int k = 0; k < 9; ++k) part[l][k] = s[k];
    part[l][9] = (double)mine;                                         // counts below 2^24: exact in any order
    tree_sum<10>(part, l);
    if (l != 0) return;
    double sum[9], out[36];
#pragma unroll
    for (int k = 0; k < 9; ++k) sum[k] = part[0][k];
    const int n = (int)part[0][9];
    info_fill(sum, n, out);
#pragma unroll
    for (int k = 0; k < 36; ++k) info[(long long)p * 36 + k] = out[k];
    count[p] = n;
}

constexpr int BATCH = 16;                // columns of the factor whose loads are in flight together

struct Graph {
    const int32_t* n;
    const int32_t* ecount;
    const int32_t* edge_i;
    const int32_t* edge_j;
    const double* X;
    const double* info;
    const double* T0;
    int Nmax, Emax;
};

struct Result {
    double* T;
    double* weight1;
    double* weight2;
    double* energy;
    uint8_t* kept;
    int32_t* iterations_done;
    double* last_step;
    int32_t* status;
};

// One scene's arrays, as the phases see them.
struct Scene {
    const int32_t* ei;
    const int32_t* ej;
    const double* X;
    const double* info;
    double* T;
    uint8_t* kept;
    double* lt;
    double* blocks;
    double* wbuf;
    int32_t* list;
    double* weight[2];
    double* energy;
    int32_t* iterations_done;
    double* last_step;
    int32_t* status;
    double tau2, prune;
    int iterations[2];
    int n, E, M;
};

// threadIdx.x == 0, compared where it is asked: the lane mask of a comparison made once would be held in scalar registers
// across the whole solve.
__device__ __forceinline__ bool first_lane()
{
    int l = threadIdx.x;
    asm volatile("" : "+v"(l));
    return l == 0;
}

// The edge pass under the current poses.  weights_only: the weight of every edge goes to the stage's output (after stage 2
// with f); otherwise it goes to the workspace with the edge's blocks.  stage2: a loop edge that was not kept has weight 0.
__device__ __forceinline__ void edge_pass(const Scene& sc, bool weights_only, int stage, int l)
{
    for (int e = l; e < sc.E; e += LANES) {
        const int i = clamp_index(sc.ei[e], sc.n), j = clamp_index(sc.ej[e], sc.n);
        double Ti[12], Tj[12], X[12], E[12], r[6];
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            Ti[k] = sc.T[i * 12 + k];
            Tj[k] = sc.T[j * 12 + k];
            X[k] = sc.X[(long long)e * 12 + k];
        }
        residual(Ti, Tj, X, E, r);
        const double* L = sc.info + (long long)e * 36;
        const double f = energy(L, r);
        const bool odometry = j == i + 1;
        double w = weight(f, L[0], sc.tau2, odometry);
        if (stage == 1 && !odometry && sc.kept[e] == 0) w = 0.0;
        if (weights_only) {
            sc.weight[stage][e] = w;
            if (stage == 1) sc.energy[e] = energy_out(f);
            else sc.kept[e] = (odometry || w >= sc.prune) ? 1 : 0;     // what stage 2 keeps
        } else {
            sc.wbuf[e] = w;
            if (w > 0.0) edge_blocks(E, r, L, w, sc.blocks + (long long)e * EDGE_W);
        }
    }
}

__global__ __launch_bounds__(LANES) void posegraph_kernel(Graph g, Result o, double tau2, double prune, int iterations1,
                                                          int iterations2, char* ws, Layout lay)
{
    __shared__ double sg[MSLOTS];                                      // the right-hand side
    __shared__ double sx[MSLOTS];                                      // y, then x
    __shared__ double s_piv;
    __shared__ int s_start[NMAX + 1];
    const int s = blockIdx.x, l = threadIdx.x;
    const int n = g.n[s], E = g.ecount[s];
    const int32_t* ei = g.edge_i + (long long)s * g.Emax;
    const int32_t* ej = g.edge_j + (long long)s * g.Emax;
    // the graph as it was given: a count outside its range or an edge out of place ends the scene before anything is indexed
    bool bad = n < 2 || n > g.Nmax || E < 0 || E > g.Emax;             // workgroup-uniform
    if (!bad)
        for (int e = l; e < E; e += LANES) bad = bad || !edge_ok(ei, ej, e, n);
    if (__syncthreads_or(bad)) {
        if (l == 0) o.status[s] = ST_BAD_GRAPH;
        return;
    }
    // the scene's pointers live in LDS and are read where they are used: sixteen of them do not fit the scalar registers
    __shared__ Scene sc;
    if (l == 0) {
        char* w = ws + lay.per_scene * s;
        sc.ei = ei;
        sc.ej = ej;
        sc.X = g.X + (long long)s * g.Emax * 12;
        sc.info = g.info + (long long)s * g.Emax * 36;
        sc.T = o.T + (long long)s * g.Nmax * 12;
        sc.kept = o.kept + (long long)s * g.Emax;
        sc.lt = (double*)(w + lay.lt);
        sc.blocks = (double*)(w + lay.blocks);
        sc.wbuf = (double*)(w + lay.wbuf);
        sc.list = (int32_t*)(w + lay.list);
        sc.weight[0] = o.weight1 + (long long)s * g.Emax;
        sc.weight[1] = o.weight2 + (long long)s * g.Emax;
        sc.energy = o.energy + (long long)s * g.Emax;
        sc.iterations_done = o.iterations_done + 2 * s;
        sc.last_step = o.last_step + 2 * s;
        sc.status = o.status + s;
        sc.tau2 = tau2;
        sc.prune = prune;
        sc.iterations[0] = iterations1;
        sc.iterations[1] = iterations2;
        sc.n = n;
        sc.E = E;
        sc.M = 6 * (n - 1);
    }
    __syncthreads();
    const int M = sc.M;
    double* lt = (double*)(ws + lay.per_scene * s + lay.lt);           // from the argument itself: global loads, not flat ones

    // the start poses; the incidence lists: node a's edges in ascending edge index (integers only)
    for (int k = l; k < n * 12; k += LANES) sc.T[k] = g.T0[(long long)s * g.Nmax * 12 + k];
    if (l < n) {
        int deg = 0;
        for (int e = 0; e < E; ++e) deg += (ei[e] == l || ej[e] == l) ? 1 : 0;
        s_start[l + 1] = deg;
    }
    __syncthreads();
    if (l == 0) {
        s_start[0] = 0;
        for (int a = 0; a < n; ++a) s_start[a + 1] += s_start[a];
    }
    __syncthreads();
    if (l < n) {
        int at = s_start[l];
        for (int e = 0; e < E; ++e)
            if (ei[e] == l || ej[e] == l) sc.list[at++] = e;
    }
    __syncthreads();

    // rows M .. Ms of a column are padding: zeros that the lanes beyond the system carry along, so that no loop needs a
    // per-lane bound
    const int Ms = (M + LANES - 1) / LANES * LANES;
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) sg[l + c * LANES] = 0.0;
    __syncthreads();
    int status = ST_OK;
    for (int stage = 0; stage < 2; ++stage) {
        const int iterations = sc.iterations[stage];
        int done = 0;
        double last = 0.0;
        for (int it = 0;; ++it) {
            // the last turn is the weight pass under the stage's final poses; a scene that ended early goes straight to it
            const bool weights_only = it >= iterations || status != ST_OK;
            edge_pass(sc, weights_only, stage, l);
            if (weights_only) break;
            for (int k = l; k < M * Ms; k += LANES) lt[k] = 0.0;
            __syncthreads();
            // the diagonal blocks' lower triangles and the right-hand side: 42 entries per unknown fragment
            for (int t = l; t < (n - 1) * 42; t += LANES) {
                const int a = 1 + t / 42, q = t % 42;
                const int r = q < 36 ? q / 6 : q - 36, c = q < 36 ? q % 6 : 0;
                if (q < 36 && r < c) continue;
                double sum = 0.0;
                for (int at = s_start[a]; at < s_start[a + 1]; ++at) {
                    const int e = clamp_index(sc.list[at], E);
                    if (!(sc.wbuf[e] > 0.0)) continue;
                    const double* blk = sc.blocks + (long long)e * EDGE_W;
                    const bool first = sc.ei[e] == a;
                    sum += q < 36 ? blk[(first ? B_II : B_JJ) + 6 * r + c] : blk[(first ? G_I : G_J) + r];
                }
                if (q < 36) lt[(6 * (a - 1) + c) * Ms + 6 * (a - 1) + r] = sum;
                else sg[6 * (a - 1) + r] = sum;
            }
            // block (j, i) is its one edge's
            for (int t = l; t < E * 36; t += LANES) {
                const int e = t / 36, q = t % 36, r = q / 6, c = q % 6;
                const int i = clamp_index(sc.ei[e], n), j = clamp_index(sc.ej[e], n);
                if (i >= 1 && sc.wbuf[e] > 0.0)
                    lt[(6 * (i - 1) + c) * Ms + 6 * (j - 1) + r] = sc.blocks[(long long)e * EDGE_W + B_JI + q];
            }
            __syncthreads();

            // H = L L': entry (i, j) is H_ij minus L_ik L_jk in ascending k, over the pivot
            for (int j = 0; j < M && status == ST_OK; ++j) {
                double v[CHUNKS];
                bool any = false;
#pragma unroll
                for (int c = 0; c < CHUNKS; ++c) {
                    const int i = l + c * LANES;
                    const bool on = i >= j && c * LANES < Ms;
                    v[c] = on ? lt[j * Ms + i] : 0.0;
                    any = any || on;
                }
                if (any) {
                    // BATCH columns' loads are issued before the first is used: a chain of single loads waits on the L2 each
                    // time.  A lane's rows that are not part of the column read the pivot's row instead and are never stored.
                    int at[CHUNKS];
#pragma unroll
                    for (int c = 0; c < CHUNKS; ++c) at[c] = (l + c * LANES >= j && c * LANES < Ms) ? l + c * LANES : j;
                    int k = 0;
                    for (; k + BATCH <= j; k += BATCH) {
                        double a[BATCH][CHUNKS], b[BATCH];
#pragma unroll
                        for (int u = 0; u < BATCH; ++u) {
                            const double* col = lt + (k + u) * Ms;
                            b[u] = col[j];
#pragma unroll
                            for (int c = 0; c < CHUNKS; ++c) a[u][c] = col[at[c]];
                        }
#pragma unroll
                        for (int u = 0; u < BATCH; ++u)
#pragma unroll
                            for (int c = 0; c < CHUNKS; ++c) v[c] -= a[u][c] * b[u];
                    }
                    for (; k < j; ++k) {
                        const double* col = lt + k * Ms;
                        const double ljk = col[j];
#pragma unroll
                        for (int c = 0; c < CHUNKS; ++c) v[c] -= col[at[c]] * ljk;
                    }
                }
#pragma unroll
                for (int c = 0; c < CHUNKS; ++c)
                    if (l + c * LANES == j) s_piv = v[c];
                __syncthreads();
                const double d = s_piv;
                if (!(finite(d) && d > 0.0)) {
                    status = ST_PIVOT;                                 // every lane reads the same d
                } else {
                    const double piv = sqrt(d);
#pragma unroll
                    for (int c = 0; c < CHUNKS; ++c) {
                        const int i = l + c * LANES;
                        if (i >= j && c * LANES < Ms) lt[j * Ms + i] = i == j ? piv : v[c] / piv;
                    }
                }
                __syncthreads();
            }
            if (status != ST_OK) continue;

            // L y = g in ascending order, L' x = y in descending order
            double v[CHUNKS];
#pragma unroll
            for (int c = 0; c < CHUNKS; ++c) v[c] = sg[l + c * LANES];
            for (int k = 0; k < M; ++k) {
                const double* col = lt + k * Ms;
#pragma unroll
                for (int c = 0; c < CHUNKS; ++c)
                    if (l + c * LANES == k) { v[c] = v[c] / col[k]; sx[k] = v[c]; }
                __syncthreads();
                const double yk = sx[k];
#pragma unroll
                for (int c = 0; c < CHUNKS; ++c) {
                    const int i = l + c * LANES;
                    if (i > k && c * LANES < Ms) v[c] -= col[i] * yk;
                }
            }
            __syncthreads();                                           // y_(M-1) is read before x_(M-1) takes its slot
            for (int k = M - 1; k >= 0; --k) {
#pragma unroll
                for (int c = 0; c < CHUNKS; ++c)
                    if (l + c * LANES == k) { v[c] = v[c] / lt[k * Ms + k]; sx[k] = v[c]; }
                __syncthreads();
                const double xk = sx[k];
#pragma unroll
                for (int c = 0; c < CHUNKS; ++c) {
                    const int i = l + c * LANES;
                    if (i < k) v[c] -= lt[i * Ms + k] * xk;
                }
            }
            // delta = -x, a fragment's six to its lane: finite, and no angle beyond a half turn
            bool inf = false, far = false;
            double d[6];
            const bool mine = l >= 1 && l < n;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                d[k] = mine ? -sx[6 * (l - 1) + k] : 0.0;
                inf = inf || !finite(d[k]);
                far = far || (k >= 3 && fabs(d[k]) > PI);
            }
            if (__syncthreads_or(inf)) status = ST_NOT_FINITE;
            else if (__syncthreads_or(far)) status = ST_ANGLE;
            if (status != ST_OK) continue;
            if (mine) {
                double T[12];
#pragma unroll
                for (int k = 0; k < 12; ++k) T[k] = sc.T[l * 12 + k];
                apply_update(T, d);
#pragma unroll
                for (int k = 0; k < 12; ++k) sc.T[l * 12 + k] = T[k];
            }
            last = 0.0;                                                // every lane: the same reads, no lane to single out
            for (int k = 0; k < M; ++k) last = max_nan(last, fabs(sx[k]));
            done = it + 1;
            __syncthreads();
        }
        if (first_lane()) {
            sc.iterations_done[stage] = done;
            sc.last_step[stage] = last;
        }
        __syncthreads();
    }
    if (first_lane()) *sc.status = status;
}

}  // namespace

extern "C" int usip_icp_information_f32(const float* rows, int row_len, const int64_t* offsets, int num_frags,
                                        long long total_rows, const int32_t* frag1, const int32_t* frag2, const int32_t* idx,
                                        const double* d2, const uint8_t* mask, int P, int Lmax, double radius, double* info,
                                        int32_t* count, void* stream)
{
    if (!bank_ok(rows, row_len, offsets, num_frags, total_rows, P, Lmax) || !(radius > 0.0)) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!frag1 || !frag2 || !idx || !d2 || !info || !count) return USIP_EINVAL;
    USIP_LAUNCH(icp_information_kernel, dim3(P), dim3(LANES), 0, (hipStream_t)stream, rows, row_len, offsets, num_frags,
                total_rows, frag1, frag2, idx, d2, mask, radius, radius_sq_hi(radius), Lmax, info, count);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" long long usip_posegraph_workspace_bytes(int S, int Nmax, int Emax)
{
    if (!shape_ok(S, Nmax, Emax)) return USIP_EINVAL;
    return Layout(S, Nmax, Emax).bytes;
}

extern "C" int usip_posegraph_optimize_f64(const int32_t* n, const int32_t* ecount, const int32_t* edge_i,
                                           const int32_t* edge_j, const double* X, const double* info, const double* T0,
                                           int S, int Nmax, int Emax, double tau2, double prune, int iterations1,
                                           int iterations2, void* workspace, long long workspace_bytes, double* T,
                                           double* weight1, double* weight2, double* energy, uint8_t* kept,
                                           int32_t* iterations_done, double* last_step, int32_t* status, void* stream)
{
    if (!shape_ok(S, Nmax, Emax) || !(tau2 > 0.0) || !(tau2 - tau2 == 0.0) || !(prune >= 0.0 && prune <= 1.0) ||
        iterations1 < 0 || iterations1 > MAX_ITERATIONS || iterations2 < 0 || iterations2 > MAX_ITERATIONS)
        return USIP_EINVAL;
    if (S == 0) return USIP_OK;
    const Layout lay(S, Nmax, Emax);
    if (!n || !ecount || !edge_i || !edge_j || !X || !info || !T0 || !workspace || workspace_bytes < lay.bytes || !T ||
        !weight1 || !weight2 || !energy || !kept || !iterations_done || !last_step || !status)
        return USIP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const size_t SE = (size_t)S * Emax;
    hipError_t e = hipMemsetAsync(T, 0, (size_t)S * Nmax * 12 * sizeof(double), st);     // zeros beyond n and ecount
    if (e == hipSuccess) e = hipMemsetAsync(weight1, 0, SE * sizeof(double), st);
    if (e == hipSuccess) e = hipMemsetAsync(weight2, 0, SE * sizeof(double), st);
    if (e == hipSuccess) e = hipMemsetAsync(energy, 0, SE * sizeof(double), st);
    if (e == hipSuccess) e = hipMemsetAsync(kept, 0, SE, st);
    if (e == hipSuccess) e = hipMemsetAsync(iterations_done, 0, (size_t)S * 2 * sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(last_step, 0, (size_t)S * 2 * sizeof(double), st);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, (size_t)S * sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    const Graph g{n, ecount, edge_i, edge_j, X, info, T0, Nmax, Emax};
    const Result o{T, weight1, weight2, energy, kept, iterations_done, last_step, status};
    USIP_LAUNCH(posegraph_kernel, dim3(S), dim3(LANES), 0, st, g, o, tau2, prune, iterations1, iterations2,
                (char*)workspace, lay);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
