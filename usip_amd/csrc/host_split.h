// usip_amd/csrc/host_split.h -- the one thread split of the host twins (csrc/*_cpu.cpp): body(lo, hi) over [0, total) in
// contiguous ranges on 1 .. 64 threads.  One thread runs inline, an empty range is never started.  Every twin's items are
// independent (each writes its own outputs, sums stay inside an item), so the partition cannot change a result: the "thread
// counts agree" tests of every twin are the check.  csrc/host_cpu.cpp's index_max keeps its own split: it mirrors the
// reference's partition.  Host only.
#pragma once
#include <thread>
#include <vector>

namespace usip_host {

inline int clamp_threads(int num_threads) { return num_threads < 1 ? 1 : (num_threads > 64 ? 64 : num_threads); }

// body(lo, hi, w): w < clamp_threads(num_threads) numbers the range, for a result slot per range
template <class F>
void split_numbered(long long total, int num_threads, const F& body)
{
    const int nt = clamp_threads(num_threads);
    if (nt == 1 || total < 2) {
        if (total > 0) body(0LL, total, 0);
        return;
    }
    std::vector<std::thread> pool;
    for (int w = 0; w < nt; ++w) {
        const long long lo = total * w / nt, hi = total * (w + 1) / nt;
        if (lo < hi) pool.emplace_back([=, &body] { body(lo, hi, w); });
    }
    for (auto& th : pool) th.join();
}

template <class F>
void split(long long total, int num_threads, const F& body)
{
    split_numbered(total, num_threads, [&body](long long lo, long long hi, int) { body(lo, hi); });
}

}  // namespace usip_host
