// usip_amd/csrc/sift_cpu.cpp -- host twin of csrc/sift.hip: the same arithmetic (csrc/sift_math.h) on host
// pointers.  The voxel average sorts the keys itself (std::stable_sort: equal keys stay in ascending input index); the scale
// space and the 25 nearest offer EVERY point of the frame to every query, in the frame's own stable order along x (no
// permutation is handed in) -- the order the contract fixes for the sums, and what the device's pruned walks must reproduce
// bit for bit.  Threads split the queries (the cells), nothing else.  Never reached from the device entry points.
#include <algorithm>
#include <cmath>
#include <vector>
#include "frames_host.h"
#include "bank.h"
#include "sift_math.h"
#include "../../include/usip_hip.h"

using namespace usip_sift;
using usip_host::for_each_query;
using usip_host::split;

namespace {

// sf: the field in the frame's sorted order
template <int S>
void dog_frame(const float* x, const float* y, const float* z, const usip_host::SortedFrame& F, const float* sf, int N,
               const Scales& sc, double* out, int num_threads)
{
    for_each_query(F.n, num_threads, [=, &F, &sc](int i) {
        const double xi = (double)x[i], yi = (double)y[i], zi = (double)z[i];
        ScaleSums<S> g;
        g.clear();
        for (int s = 0; s < F.n; ++s) g.offer(xi, yi, zi, F.x[s], F.y[s], F.z[s], sf[s], sc);
        g.dog(out + i, N);
    });
}

template <int S>
void extrema_frame(const double* d, const int32_t* idx, int n, int N, double min_contrast, uint8_t* mask, int32_t* scale,
                   int num_threads)
{
    split(n, num_threads, [=](long long lo, long long hi) {
        for (long long i = lo; i < hi; ++i) {
            Extrema<S> e;
            e.clear();
            for (int k = 0; k < NEAREST; ++k) e.offer(d + usip_bank::safe_index(idx[i * NEAREST + k], n), N);
            const int found = e.decide(d + i, N, min_contrast);
            mask[i] = found ? 1 : 0;
            scale[i] = found;
        }
    });
}

}  // namespace

extern "C" int usip_sift_voxel_keys_f32_cpu(const float* pc, const int32_t* count, int B, int N, double leaf, int64_t* keys)
{
    if (bad_frames(B, N) || !(leaf > 0.0) || !is_finite(leaf) || !pc || !keys) return USIP_EINVAL;
    for (int f = 0; f < B; ++f) {
        const float *x = pc + 3LL * f * N, *y = x + N, *z = y + N;
        const int c = count ? count[f] : N;
        for (int i = 0; i < N; ++i) keys[(long long)f * N + i] = i < c ? cell_key(x[i], y[i], z[i], leaf) : DEAD_KEY;
    }
    return USIP_OK;
}

extern "C" int usip_sift_voxel_average_f32_cpu(const float* pc, const float* field, int axis, const int64_t* keys, int B, int N,
                                               float* out_pc, float* out_field, int32_t* count_out, int num_threads)
{
    if (bad_frames(B, N) || axis < 0 || axis > 2 || !pc || !keys || !out_pc || !out_field || !count_out) return USIP_EINVAL;
    std::vector<int32_t> order(N), heads;
    for (int f = 0; f < B; ++f) {
        const float *x = pc + 3LL * f * N, *y = x + N, *z = y + N;
        const float* fl = field ? field + (long long)f * N : nullptr;
        const int64_t* k = keys + (long long)f * N;
        float *ox = out_pc + 3LL * f * N, *oy = ox + N, *oz = oy + N, *of = out_field + (long long)f * N;
        for (int i = 0; i < N; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return k[a] < k[b]; });
        heads.clear();
        for (int s = 0; s < N; ++s)
            if (k[order[s]] != DEAD_KEY && (s == 0 || k[order[s]] != k[order[s - 1]])) heads.push_back(s);
        const int total = (int)heads.size();
        const int32_t *ord = order.data(), *hd = heads.data();
        split(total, num_threads, [=](long long lo, long long hi) {
            for (long long row = lo; row < hi; ++row) {
                CellSum cell;
                const int64_t key = k[ord[hd[row]]];
                for (int s = hd[row]; s < N && k[ord[s]] == key; ++s) {
                    const int j = ord[s];
                    cell.add(x[j], y[j], z[j], fl ? fl[j] : 0.0f);
                }
                cell.centroid(fl != nullptr, axis, ox + row, oy + row, oz + row, of + row);
            }
        });
        for (int q = total; q < N; ++q) { ox[q] = 0.0f; oy[q] = 0.0f; oz[q] = 0.0f; of[q] = 0.0f; }
        count_out[f] = total;
    }
    return USIP_OK;
}

extern "C" int usip_sift_dog_f32_cpu(const float* pc, const float* field, const int32_t* count, int B, int N, int S,
                                     const double* sigma2, double* dog, int num_threads)
{
    if (bad_frames(B, N) || !good_scales(sigma2, S) || !pc || !field || !dog) return USIP_EINVAL;
    const Scales sc = make_scales(sigma2, S);
    usip_host::SortedFrame F(N);
    std::vector<float> sf(N);
    for (int f = 0; f < B; ++f) {
        const float *x = pc + 3LL * f * N, *y = x + N, *z = y + N;
        double* out = dog + (long long)f * (S - 1) * N;
        const int n = octave_points(count, f, N);
        for (int s = 0; s + 1 < S; ++s)
            for (int i = n; i < N; ++i) out[(long long)s * N + i] = 0.0;
        F.sort(x, y, z, n);
        F.gather(field + (long long)f * N, sf.data());
#define USIP_SIFT_DOG(s) dog_frame<s>(x, y, z, F, sf.data(), N, sc, out, num_threads)
        USIP_SIFT_DISPATCH(S, USIP_SIFT_DOG)
#undef USIP_SIFT_DOG
    }
    return USIP_OK;
}

extern "C" int usip_sift_exp_f64_cpu(const double* x, long long n, double* out)
{
    if (n < 0 || !x || !out) return USIP_EINVAL;
    for (long long i = 0; i < n; ++i) out[i] = sift_exp(x[i]);
    return USIP_OK;
}

extern "C" int usip_sift_nearest_f32_cpu(const float* pc, const int32_t* count, int B, int N, int32_t* idx, int num_threads)
{
    if (bad_frames(B, N) || !pc || !idx) return USIP_EINVAL;
    usip_host::SortedFrame F(N);
    for (int f = 0; f < B; ++f) {
        const float *x = pc + 3LL * f * N, *y = x + N, *z = y + N;
        int32_t* out = idx + (long long)f * N * NEAREST;
        const int n = octave_points(count, f, N);
        for (long long i = (long long)n * NEAREST; i < (long long)N * NEAREST; ++i) out[i] = 0;
        F.sort(x, y, z, n);
        for_each_query(n, num_threads, [=, &F](int i) {
            const double xi = (double)x[i], yi = (double)y[i], zi = (double)z[i];
            usip_prep::KList<NEAREST> list;
            list.clear();
            for (int s = 0; s < n; ++s) {
                const double d = usip_prep::sqdist(xi, yi, zi, F.x[s], F.y[s], F.z[s]);
                if (list.admits(d, F.order[s])) list.insert(d, F.order[s]);
            }
            for (int k = 0; k < NEAREST; ++k) out[(long long)i * NEAREST + k] = list.j[k];
        });
    }
    return USIP_OK;
}

extern "C" int usip_sift_extrema_f32_cpu(const double* dog, const int32_t* idx, const int32_t* count, int B, int N, int S,
                                         double min_contrast, uint8_t* mask, int32_t* scale_index, int num_threads)
{
    if (bad_frames(B, N) || S < SCALES_MIN || S > SCALES_MAX || !(min_contrast >= 0.0) || !dog || !idx || !mask || !scale_index)
        return USIP_EINVAL;
    for (int f = 0; f < B; ++f) {
        const double* d = dog + (long long)f * (S - 1) * N;
        const int32_t* nb = idx + (long long)f * N * NEAREST;
        uint8_t* m = mask + (long long)f * N;
        int32_t* sc = scale_index + (long long)f * N;
        const int n = octave_points(count, f, N);
        for (int i = n; i < N; ++i) { m[i] = 0; sc[i] = 0; }
#define USIP_SIFT_EXTREMA(s) extrema_frame<s>(d, nb, n, N, min_contrast, m, sc, num_threads)
        USIP_SIFT_DISPATCH(S, USIP_SIFT_EXTREMA)
#undef USIP_SIFT_EXTREMA
    }
    return USIP_OK;
}
