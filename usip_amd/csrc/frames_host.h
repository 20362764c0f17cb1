// usip_amd/csrc/frames_host.h -- the frame loop of the baseline detectors' host twins (csrc/iss_cpu.cpp, csrc/harris_cpu.cpp,
// csrc/sift_cpu.cpp): a frame's live points in its stable order along x, and the split of its queries over threads.  A twin
// that sums offers EVERY sorted row to every query in that order -- the order the contracts fix, and what the device's pruned
// walks over the caller's permutation must reproduce bit for bit.  Host only.
#pragma once
#include <algorithm>
#include <vector>
#include "host_split.h"
#include "iss_math.h"

namespace usip_host {

using usip_iss::live_points;

// order[0 .. n): the frame's live points ascending along x, ties towards the lower index
inline void sort_along_x(const float* x, int n, std::vector<int32_t>& order)
{
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.begin() + n, [&](int32_t a, int32_t b) { return x[a] < x[b]; });
}

// One frame of at most N points in that order: x, y, z of sorted position s < n, and order[s], the row it came from
struct SortedFrame {
    std::vector<float> xyz;
    std::vector<int32_t> order;
    const float *x, *y, *z;
    int n = 0;
    explicit SortedFrame(int N) : xyz(3 * (size_t)N), order(N), x(xyz.data()), y(x + N), z(y + N) {}
    void sort(const float* px, const float* py, const float* pz, int live)
    {
        n = live;
        sort_along_x(px, n, order);
        gather(px, xyz.data());
        gather(py, xyz.data() + order.size());
        gather(pz, xyz.data() + 2 * order.size());
    }
    // a plane of the caller's beside them: to[s] = from[order[s]]
    template <class T>
    void gather(const T* from, T* to) const
    {
        for (int s = 0; s < n; ++s) to[s] = from[order[s]];
    }
};

// fn(i) for every query i < n, on up to num_threads threads
template <class F>
void for_each_query(int n, int num_threads, const F& fn)
{
    split(n, num_threads, [&fn](long long lo, long long hi) {
        for (long long i = lo; i < hi; ++i) fn((int)i);
    });
}

}  // namespace usip_host
