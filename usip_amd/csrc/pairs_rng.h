// usip_amd/csrc/pairs_rng.h -- counter-based randomness of the training-pair builder, compiled both by the
// device code (csrc/pairs.hip) and by the host twin (csrc/pairs_cpu.cpp), so that both draw exactly the same bits.
//
//   philox4x64_10   Random123's Philox4x64-10 (Salmon et al., SC'11), the generator numpy ships as np.random.Philox:
//                   tests/test_pairs_cpu.py checks it block for block against numpy.
//   pairs_block     the block of one draw: key = (seed, 0), counter = (element, stream tag, global pair, step), so a
//                   pair's data depends on (seed, step, rank * P + p) only -- never on the world size.
//   u53 / normal4   float64 uniforms from 53 random bits; standard normals by Box-Muller (two per pair of uniforms).
//   PairsPerm       a keyed bijection on [0, n): a balanced Feistel network over the next even-bit power of two with
//                   cycle-walking (the construction of thrust::shuffle).  perm(j) is an O(1) draw without replacement,
//                   in random order, with no sort and no scratch.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define USIP_HD __host__ __device__ __forceinline__
#else
#define USIP_HD inline
#endif

namespace usip_pairs {

USIP_HD void mulhilo64(uint64_t a, uint64_t b, uint64_t& hi, uint64_t& lo)
{
#if defined(__HIP_DEVICE_COMPILE__)
    lo = a * b;
    hi = __umul64hi(a, b);
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    lo = (uint64_t)p;
    hi = (uint64_t)(p >> 64);
#endif
}

// out = Philox4x64-10(ctr, key)
USIP_HD void philox4x64_10(const uint64_t ctr[4], const uint64_t key[2], uint64_t out[4])
{
    uint64_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r > 0) { k0 += 0x9E3779B97F4A7C15ull; k1 += 0xBB67AE8584CAA73Bull; }
        uint64_t hi0, lo0, hi1, lo1;
        mulhilo64(0xD2E7470EE14C6C93ull, c0, hi0, lo0);
        mulhilo64(0xCA5A826395121157ull, c2, hi1, lo1);
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Stream tags (counter word 1 = tag << 8 | cloud, cloud 0 = src, 1 = dst).
enum : uint32_t {
    TAG_CHOICE = 1,     // round keys of the subsample bijection over the scan's rows
    TAG_CAND = 2,       // round keys of the FPS-candidate bijection over the N slots
    TAG_FIRST = 3,      // round keys of the bijection over the candidates whose image of 0 is the first FPS index
    TAG_JIT_PC = 4,     // element = slot: normals 0..2 of the block
    TAG_JIT_SN = 5,     // element = 2 * slot + channel / 4: normal channel % 4
    TAG_JIT_NODE = 6,   // element = node: normals 0..2
    TAG_PARAM_U = 7,    // element = i / 4: uniform i % 4 of the pair's parameter draws
    TAG_PARAM_N = 8,    // element 0: augment perturbation normals, 1: transform perturbation normals
};

USIP_HD void pairs_block(uint64_t seed, uint64_t step, uint64_t gpair, uint32_t tag, uint32_t cloud, uint64_t elem,
                         uint64_t out[4])
{
    const uint64_t ctr[4] = {elem, ((uint64_t)tag << 8) | cloud, gpair, step};
    const uint64_t key[2] = {seed, 0};
    philox4x64_10(ctr, key, out);
}

// [0, 1) with 53 random bits
USIP_HD double u53(uint64_t x) { return (double)(x >> 11) * 0x1.0p-53; }

// Four standard normals from one block: Box-Muller on (u1, u2) = (words 0, 1) and (words 2, 3); u1 in (0, 1].
USIP_HD void normal4(const uint64_t b[4], double z[4])
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const double u1 = (double)((b[2 * h] >> 11) + 1) * 0x1.0p-53;
        const double t = 6.283185307179586 * u53(b[2 * h + 1]);
        const double r = sqrt(-2.0 * log(u1));
        z[2 * h] = r * cos(t);
        z[2 * h + 1] = r * sin(t);
    }
}

USIP_HD uint32_t hash32(uint32_t x)          // "lowbias32" (C. Wellons): a full-avalanche 32-bit mix
{
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// Keyed permutation of [0, n), n <= 2^32: eight balanced Feistel rounds over 2^(2h) >= n, cycle-walking the images >= n
// (at most 4n/n = 4 steps expected; the walk ends because a permutation's cycle through j < n returns below n).
struct PairsPerm {
    uint32_t key[8];
    uint32_t half, mask;
    uint64_t n;

    USIP_HD void init(const uint64_t b[4], uint64_t n_)
    {
        n = n_;
#pragma unroll
        for (int i = 0; i < 4; ++i) { key[2 * i] = (uint32_t)b[i]; key[2 * i + 1] = (uint32_t)(b[i] >> 32); }
        uint32_t bits = 2;
        while (bits < 64 && (1ull << bits) < n) bits += 2;
        half = bits / 2;
        mask = half >= 32 ? 0xffffffffu : ((1u << half) - 1u);
    }
    USIP_HD uint64_t round_trip(uint64_t x) const
    {
        uint32_t l = (uint32_t)(x >> half) & mask, r = (uint32_t)x & mask;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t f = hash32(r ^ key[i]) & mask;
            const uint32_t t = l ^ f;
            l = r;
            r = t;
        }
        return ((uint64_t)l << half) | r;
    }
    USIP_HD uint64_t operator()(uint64_t j) const
    {
        uint64_t x = round_trip(j);
        while (x >= n) x = round_trip(x);
        return x;
    }
};

}  // namespace usip_pairs
