// usip_amd/csrc/keypoints_host.h -- the keypoint loop of the baseline descriptors' host twins (csrc/fpfh_cpu.cpp,
// csrc/shot_cpu.cpp, csrc/spin_cpu.cpp) over csrc/frames_host.h.  A keypoint (any position) tests ALL live points of its frame
// in the frame's stable order along x (the twin's own sort, no permutation is handed in) -- what the device's wave per keypoint
// (csrc/keypoint_walk.h) does over its pruned window.  Integer sums are free of the order.  A float64 sum takes the contract's:
// 64 partial sums, the one of lane l over the sorted positions lo + l + 64 k ascending, lo = first_within() -- the phase of the
// lane assignment (s - lo) % LANES --, folded by the xor-butterfly 32 .. 1 (fold_lanes).  Threads split the keypoints, nothing
// else.  Host only.
#pragma once
#include "fpfh_math.h"
#include "frames_host.h"

namespace usip_host {

using usip_fpfh::LANES;

// lanes[0] = the 64 partials folded as the device's xor-butterfly 32 .. 1 folds them; add(a, b) is a += b
template <class T, class Add>
void fold_lanes(T* lanes, const Add& add)
{
    for (int off = LANES / 2; off >= 1; off >>= 1)
        for (int l = 0; l < off; ++l) add(lanes[l], lanes[l + off]);
}

// One frame in its order along x with, where the twin reads them, its normals in that order: n0[s], n1[s], n2[s]
struct DescribedFrame : SortedFrame {
    std::vector<double> normal;
    const double *n0 = nullptr, *n1 = nullptr, *n2 = nullptr;
    int f = 0;
    DescribedFrame(int N, bool normals) : SortedFrame(N), normal(normals ? 3 * (size_t)N : 0) {}
    // frame `frame` of pc f32 [B][3][N] and, with normals, of normals f64 [B][3][N]
    void sort(const float* pc, const int32_t* count, const double* normals, int frame)
    {
        const long long N = (long long)order.size();
        f = frame;
        const float* px = pc + 3 * f * N;
        SortedFrame::sort(px, px + N, px + 2 * N, live_points(count, f, (int)N));
        if (normal.empty()) return;
        const double* from = normals + 3 * f * N;
        double* to = normal.data();
        for (int c = 0; c < 3; ++c) gather(from + c * N, to + c * N);
        n0 = to;
        n1 = to + N;
        n2 = to + 2 * N;
    }
};

// An output [B][M][width] of a keypoint twin: the row of slot = f * M + q
template <class T>
struct Rows {
    T* base;
    int width;
    Rows(T* base_, int width_) : base(base_), width(width_) {}
    T* operator[](long long slot) const { return base + width * slot; }
    void zero(long long slot) const { std::fill_n((*this)[slot], width, T(0)); }
};

// Per frame: zeros in the slots beyond kp_count[f] of every output, the sort (normals, where not null, beside it), and
// fn(S, slot, qx, qy, qz) for the live keypoints q, slot = f * M + q, on up to num_threads threads
template <class Fn, class... T>
void for_each_keypoint(const float* pc, const int32_t* count, const double* normals, const float* keypoints,
                       const int32_t* kp_count, int B, int N, int M, int num_threads, const Fn& fn, Rows<T>... outs)
{
    DescribedFrame S(N, normals != nullptr);
    for (int f = 0; f < B; ++f) {
        const float* kp = keypoints + 3LL * f * M;
        const long long first = (long long)f * M;
        const int m = live_points(kp_count, f, M);
        for (int q = m; q < M; ++q) (outs.zero(first + q), ...);
        S.sort(pc, count, normals, f);
        for_each_query(m, num_threads, [&, kp, first](int q) {
            fn(S, first + q, (double)kp[q], (double)kp[M + q], (double)kp[2LL * M + q]);
        });
    }
}

}  // namespace usip_host
