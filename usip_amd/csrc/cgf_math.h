// usip_amd/csrc/cgf_math.h -- the CGF triplet loss of the indoor descriptor (the reference's
// losses.DescCGFLoss, models/losses.py:240-314): the arithmetic the device kernels (csrc/cgf_loss.hip) and the host twin
// (csrc/cgf_loss_cpu.cpp) share, so both decide and round alike.  include/usip_hip.h, section f-22, is the contract.
//
//   selection   float32, as the reference decides: d = sqrtf((dx dx + dy dy) + dz dz), never contracted; positive when d <=
//               (float)radius, outside when d > (float)radius (a NaN distance is neither).  Three running candidates per
//               anchor, each a (key, j): j_pos the arg-max of (positive ? u1 : 0), j_far the arg-min of the float32 sum d +
//               (positive ? 1000.f : 0.f), j_out the arg-max of (outside ? u2 : 0).  `wins` is a total order on (key, j) with
//               the lowest j first among equal keys, so any split of the row over lanes or threads gives one answer; a NaN
//               key never wins, and a row without a winner gives 0.
//   draws       explicit float32 arrays, or Philox4x64-10 (csrc/pairs_rng.h) with key (seed, KEY_WORD):
//                 counter (i << 16 | j, TAG_CGF << 8 | 0, global batch element, step): word 0 -> u1_ij, word 1 -> u2_ij
//                 counter (i,           TAG_CGF << 8 | 1, global batch element, step): word 0 -> u3_i
//               a uniform is the word's top 24 bits times 2^-24: exact in float32, in [0, 1).  M <= 65535 keeps i << 16 | j
//               inside 32 bits.  Nothing else enters a draw: not B, not the rank split, not the launch geometry.
//   distances   float64 from the float32 descriptors: lane l of 64 adds (a_c - p_c)^2 over c = l, l + 64, ... ascending, the
//               64 partial sums go through the binary tree (part[l] += part[l + s], s = 32 .. 1), then one sqrt.
//   row         per batch element, ROW_LANES partial sums of the weights (lane l adds i = l, l + ROW_LANES, ...), the same
//               kind of tree, then the row's values anchor by anchor.
#pragma once
#include "pairs_rng.h"

namespace usip_cgf {

constexpr uint32_t TAG_CGF = 27;                   // continues the stream tags (1-10 the builders and evaluations, 23-26 f-8)
constexpr uint64_t KEY_WORD = 0x6367665f6c6f7373ull;   // "cgf_loss": the second Philox key word
constexpr int LANES = 64;
constexpr int ROW_LANES = 256;
constexpr int MAX_M = 65535, MAX_C = 4096;
constexpr int NONE = 0x7fffffff;                   // the j of a candidate nobody has claimed yet
constexpr float FAR_SHIFT = 1000.f;                // models/losses.py:283
constexpr double ACTIVE_EPS = 1e-5;                // models/losses.py:306

USIP_HD bool bad_shape(int B, int M) { return B < 1 || M < 1 || M > MAX_M; }
USIP_HD bool bad_channels(int C) { return C < 1 || C > MAX_C; }
USIP_HD bool bad_radius(double radius) { return !(radius > 0.0) || !((float)radius > 0.f); }
USIP_HD int clamp_index(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// ---------------------------------------------------------------------------------------------- draws
USIP_HD float u24(uint64_t word) { return (float)(uint32_t)(word >> 40) * 0x1.0p-24f; }

USIP_HD void draw_pair(uint64_t seed, uint64_t step, uint64_t gelem, int i, int j, float& u1, float& u2)
{
    const uint64_t ctr[4] = {((uint64_t)(uint32_t)i << 16) | (uint64_t)(uint32_t)j, (uint64_t)TAG_CGF << 8, gelem, step};
    const uint64_t key[2] = {seed, KEY_WORD};
    uint64_t out[4];
    usip_pairs::philox4x64_10(ctr, key, out);
    u1 = u24(out[0]);
    u2 = u24(out[1]);
}

USIP_HD float draw_anchor(uint64_t seed, uint64_t step, uint64_t gelem, int i)
{
    const uint64_t ctr[4] = {(uint64_t)(uint32_t)i, ((uint64_t)TAG_CGF << 8) | 1u, gelem, step};
    const uint64_t key[2] = {seed, KEY_WORD};
    uint64_t out[4];
    usip_pairs::philox4x64_10(ctr, key, out);
    return u24(out[0]);
}

// ---------------------------------------------------------------------------------------------- selection
struct Cand {
    float key;
    int j;
};

// a before b in the arg-max order: the larger key, the lower j among equal keys; a NaN key is never before anything
USIP_HD bool wins_max(const Cand& a, const Cand& b) { return a.key > b.key || (a.key == b.key && a.j < b.j); }
USIP_HD bool wins_min(const Cand& a, const Cand& b) { return a.key < b.key || (a.key == b.key && a.j < b.j); }

struct Picks {
    Cand pos, far, out;
    bool has;

    USIP_HD void init()
    {
        pos.key = -1.f; pos.j = NONE;
        far.key = __builtin_inff(); far.j = NONE;
        out.key = -1.f; out.j = NONE;
        has = false;
    }
    // offer candidate j of the anchor at (ax, ay, az)
    USIP_HD void offer(float ax, float ay, float az, float px, float py, float pz, float r, float u1, float u2, int j)
    {
        const float dx = ax - px, dy = ay - py, dz = az - pz;
        const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
        const bool positive = d <= r, outside = d > r;
        has = has || positive;
        const Cand cp = {positive ? u1 : 0.f, j}, cf = {d + (positive ? FAR_SHIFT : 0.f), j}, co = {outside ? u2 : 0.f, j};
        if (wins_max(cp, pos)) pos = cp;
        if (wins_min(cf, far)) far = cf;
        if (wins_max(co, out)) out = co;
    }
    USIP_HD void merge(const Picks& o)
    {
        if (wins_max(o.pos, pos)) pos = o.pos;
        if (wins_min(o.far, far)) far = o.far;
        if (wins_max(o.out, out)) out = o.out;
        has = has || o.has;
    }
};

USIP_HD int picked(const Cand& c) { return c.j == NONE ? 0 : c.j; }
USIP_HD bool takes_far(float u3) { return u3 < 0.5f; }

// ---------------------------------------------------------------------------------------------- loss
USIP_HD double sqdiff(float a, float p)
{
    const double v = (double)a - (double)p;
    return v * v;
}

USIP_HD double raw_weight(double sigma_max, float sigma)
{
    const double v = sigma_max - (double)sigma;
    return v > 0.0 ? v : 0.0;                      // a NaN sigma weighs nothing
}

USIP_HD double before_clamp(bool has, double d_pos, double d_neg, double gamma) { return has ? (d_pos - d_neg) + gamma : 0.0; }

// the row's values of one anchor from the batch element's mean raw weight and n + 1
USIP_HD void row_values(double raw, double mean, double before, int M, int n1, double& coef, float& loss)
{
    const double w = mean > 0.0 ? raw / mean : 0.0;   // every sigma at or above sigma_max: weight 0, not 0 / 0
    coef = before > 0.0 ? (w * (double)M) / (double)n1 : 0.0;
    loss = before > 0.0 ? (float)(coef * before) : 0.f;
}

// ---------------------------------------------------------------------------------------------- backward
USIP_HD double unit(float a, float p, double dist)
{
    return dist > 0.0 ? ((double)a - (double)p) / dist : 0.0;     // torch's norm backward at zero distance
}

// host form of the trees (the device walks them with shuffles or through LDS, in the same order)
template <int N>
inline double tree_sum(double* part)
{
    for (int s = N / 2; s > 0; s >>= 1)
        for (int l = 0; l < s; ++l) part[l] += part[l + s];
    return part[0];
}

}  // namespace usip_cgf
