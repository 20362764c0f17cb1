// usip_amd/csrc/cloud_stage.h -- the per-cloud launches of the two batch builders, csrc/pairs.hip and
// csrc/desc_pairs.hip (f-8): each supplies its View (csrc/pairs_math.h), its out pointers and the kernels that fill the
// tables and first FPS indices; everything per slot and per node is here, once.
//   cloud_points_kernel   one thread per slot of each of the 2P clouds (cloud_point)
//   fps_kernel            usip_fps_f32 (csrc/fps.hip) on the un-augmented candidates, unchanged
//   cloud_nodes_kernel    one thread per node (cloud_node)
#pragma once
#include "common.h"
#include "pairs_math.h"

namespace usip_pairs {

constexpr int PT = 256;

template <class Src, class View>
__global__ __launch_bounds__(PT) void cloud_points_kernel(usip_pairs_recipe r, Src src, View v, const float* __restrict__ bank,
                                                          int P, CloudOut out, float* __restrict__ cand_xyz)
{
    const int j = blockIdx.x * PT + threadIdx.x, q = blockIdx.y;
    if (j < r.N) cloud_point(r, src, v, bank, P, q, j, out, cand_xyz + (long long)q * 3 * r.n_sub);
}

template <class Src, class View>
__global__ __launch_bounds__(PT) void cloud_nodes_kernel(usip_pairs_recipe r, Src src, View v, int P,
                                                         const float* __restrict__ cand_xyz, const int32_t* __restrict__ fps,
                                                         CloudOut out)
{
    const int m = blockIdx.x * PT + threadIdx.x, q = blockIdx.y;
    if (m < r.M) cloud_node(r, src, v, P, q, m, cand_xyz + (long long)q * 3 * r.n_sub, fps + (long long)q * r.M, out);
}

inline long long align256(long long b) { return (b + 255) & ~255LL; }

struct CloudWorkspace {
    double* table;          // [tables][T_SIZE]
    float* cand_xyz;        // [2P][3][n_sub]
    int32_t* first;         // [2P]
    int32_t* fps;           // [2P][M]
};

// The four parts both builders have, in workspace-offset order: parts[0] tables, 1 candidates, 2 first indices, 3 FPS
// picks, parts[4] = the end (where a builder's own parts go on).  tables = P (one per pair) or 2P (one per cloud).
inline void cloud_workspace_layout(const usip_pairs_recipe& r, int P, long long tables, char* base, CloudWorkspace* w,
                                   long long parts[5])
{
    const long long bytes[4] = {tables * T_SIZE * 8, (long long)2 * P * 3 * r.n_sub * 4, (long long)2 * P * 4,
                                (long long)2 * P * r.M * 4};
    parts[0] = 0;
    for (int i = 0; i < 4; ++i) parts[i + 1] = parts[i] + align256(bytes[i]);
    if (w) {
        w->table = (double*)(base + parts[0]);
        w->cand_xyz = (float*)(base + parts[1]);
        w->first = (int32_t*)(base + parts[2]);
        w->fps = (int32_t*)(base + parts[3]);
    }
}

// points -> FPS -> nodes of the 2P clouds on `stream`; the tables and first indices are already enqueued there.
template <class Src, class View>
int cloud_stage_launch(const usip_pairs_recipe& r, const Src& src, const View& v, const float* bank, int P,
                       const CloudOut& out, const CloudWorkspace& w, hipStream_t stream)
{
    USIP_LAUNCH((cloud_points_kernel<Src, View>), dim3(usip_ceil_div(r.N, PT), 2 * P), dim3(PT), 0, stream, r, src, v, bank,
                P, out, w.cand_xyz);
    USIP_LAUNCH_CHECK();
    const int rc = usip_fps_f32(w.cand_xyz, w.first, w.fps, 2 * P, r.n_sub, r.M, stream);
    if (rc != USIP_OK) return rc;
    USIP_LAUNCH((cloud_nodes_kernel<Src, View>), dim3(usip_ceil_div(r.M, PT), 2 * P), dim3(PT), 0, stream, r, src, v, P,
                w.cand_xyz, w.fps, out);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

}  // namespace usip_pairs
