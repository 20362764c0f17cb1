// usip_amd/csrc/bank.h -- the view of a fragment bank (one float32 buffer of rows with int64 CSR offsets, as
// fragments.FragmentBank and RefineBank hold it) that the kernels and the host twins of f-9, f-13 and f-14 read through:
// csrc/fragments.hip, csrc/icp.hip, csrc/posegraph.hip and their *_cpu.cpp.  Host and device; nothing here does arithmetic
// on coordinates, so nothing here can move a result.  safe_index is also what csrc/prepare.hip and csrc/iss.hip put around
// every index they read from memory.
#pragma once
#include <stdint.h>

#ifndef USIP_HD
#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define USIP_HD __host__ __device__ __forceinline__
#else
#define USIP_HD inline
#endif
#endif

namespace usip_bank {

struct Range {
    long long first;
    int n;
};

// fragment f of the bank -> (first row, rows), never outside the buffer and never more than lmax rows
USIP_HD Range fragment_range(const int64_t* offsets, int num_frags, long long total, int f, int lmax)
{
    f = f < 0 ? 0 : (f >= num_frags ? num_frags - 1 : f);
    long long lo = offsets[f], hi = offsets[f + 1];
    lo = lo < 0 ? 0 : (lo > total ? total : lo);
    hi = hi < lo ? lo : (hi > total ? total : hi);
    return {lo, (int)(hi - lo > (long long)lmax ? (long long)lmax : hi - lo)};
}

// an index read from memory: itself when it names one of n rows, otherwise row 0
USIP_HD int safe_index(int j, int n) { return (unsigned)j < (unsigned)n ? j : 0; }

struct Bank {
    const float* rows;
    const int64_t* offsets;
    int row_len, num_frags;
    long long total;
    USIP_HD Range range(int f, int lmax) const { return fragment_range(offsets, num_frags, total, f, lmax); }
};

// what every entry point that takes a bank refuses (the two ICP entries add `&& perm1`)
inline bool bank_ok(const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total, int P, int Lmax)
{
    return rows && offsets && row_len >= 3 && num_frags >= 1 && total >= 0 && P >= 0 && P <= 65535 && Lmax >= 1 &&
           Lmax <= (1 << 24);
}

}  // namespace usip_bank
