// usip_amd/csrc/cloud_stage_host.h -- host twin of csrc/cloud_stage.h for csrc/pairs_cpu.cpp and csrc/desc_pairs_cpu.cpp:
// the same cloud_point / cloud_node (csrc/pairs_math.h) in loops, with a float64 farthest-point sampling loop in numpy's
// order (FarthestSampler.sample, data/kitti_detector_loader.py:69-83, data/kitti_descriptor_loader.py:70-84).  Host only.
#pragma once
#include <cmath>
#include <vector>
#include "pairs_math.h"

namespace usip_pairs {

// out[0] = first, then k-1 times the first arg-max of the running minimum of (dx*dx + dy*dy) + dz*dz in float64
inline void fps_host(const float* pts, int n, int first, int k, int32_t* out)
{
    std::vector<double> dist((size_t)n, INFINITY);
    int cur = first;
    out[0] = cur;
    for (int it = 1; it < k; ++it) {
        const double cx = pts[cur], cy = pts[n + cur], cz = pts[2 * n + cur];
        double best = -1.0;
        int bi = 0;
        for (int j = 0; j < n; ++j) {
            const double dx = cx - (double)pts[j], dy = cy - (double)pts[n + j], dz = cz - (double)pts[2 * n + j];
            const double d = (dx * dx + dy * dy) + dz * dz;
            dist[j] = d < dist[j] ? d : dist[j];
            if (dist[j] > best) { best = dist[j]; bi = j; }
        }
        out[it] = cur = bi;
    }
}

// Cloud q of P pairs: slots -> candidates -> fps_host -> nodes.
template <class Src, class View>
void cloud_host(const usip_pairs_recipe& r, const Src& src, const View& v, const float* bank, int P, int q,
                const CloudOut& out)
{
    const int c = q / P, p = q - c * P;
    std::vector<float> cand((size_t)3 * r.n_sub);
    std::vector<int32_t> fps((size_t)r.M);
    for (int j = 0; j < r.N; ++j) cloud_point(r, src, v, bank, P, q, j, out, cand.data());
    fps_host(cand.data(), r.n_sub, src.first(p, c, r.n_sub), r.M, fps.data());
    for (int m = 0; m < r.M; ++m) cloud_node(r, src, v, P, q, m, cand.data(), fps.data(), out);
}

}  // namespace usip_pairs
