// usip_amd/csrc/ground_truth_math.h -- the arithmetic of a fragment scene's ground truth, shared by the
// kernels of csrc/ground_truth.hip and the host twin of csrc/ground_truth_cpu.cpp.  The conventions are f-9's: float32 rows,
// float64 arithmetic, never contracted, the moved point by csrc/fragments_math.h's xform, the strict sqrt(d2) < radius of
// within, sums in a fixed order (csrc/registration_math.h's tree).
//
// Reference semantics (evaluation/matlab/eval_indoor/3dmatch/getGtInfoLog.m), per pair i < j with relExt = inv(T_i) T_j:
//   nnDist                 for every row of fragment j moved by relExt, the distance d to the nearest row of fragment i
//   alignedRatio           #{d < 0.03} / (rows of fragment i)
//   corresQ                the moved rows with d < 0.006, thinned to 5000 when there are more
//   covMat                 sum over corresQ of G'G, G = [I3 | -[q]x]
// -[q]x = [0 qz -qy; -qz 0 qx; qy -qx 0] is fragments_math.h's M at 2 s = q, so G'G is info_fill over the terms below.
// The thinning is our own (MATLAB's pcdownsample 'random' draws from a stream that cannot be reproduced): every near row
// carries a 63-bit Philox key that depends on (seed, pair id, row) only, the 5000 smallest (key, row) are kept.
#pragma once
#include "fragments_math.h"

namespace usip_gt {

constexpr int LANES = 256;                          // = usip_reg::REFIT_LANES: the tree sums 256 partial sums
constexpr int CAP_MAX = 65536;                      // selected rows per pair
constexpr uint64_t KEY_WORD = 0x67745f6b6579ull;    // "gt_key": the second Philox key word of the selection stream
constexpr uint64_t KEY_NONE = ~0ull;                // a row that is not near, and the padding: sorts behind every near row
static_assert(LANES == usip_reg::REFIT_LANES, "tree_sum walks REFIT_LANES partial sums");

// 0: no row within `far`; 1: one within `far`; 2: one within `near` (far > near), from the smallest d2 of the row
USIP_HD uint8_t reach_class(double d2, double far, double far2hi, double near, double near2hi)
{
    return usip_frag::within(d2, near, near2hi) ? 2 : (usip_frag::within(d2, far, far2hi) ? 1 : 0);
}

// the selection key of a near row: 63 random bits, so it never equals KEY_NONE
USIP_HD uint64_t selection_key(uint64_t seed, uint64_t pair_id, uint64_t row)
{
    const uint64_t ctr[4] = {row, 0, pair_id, 0};
    const uint64_t key[2] = {seed, KEY_WORD};
    uint64_t out[4];
    usip_pairs::philox4x64_10(ctr, key, out);
    return out[0] >> 1;
}

// One correspondence's nine distinct terms of G'G besides the count: q, then the six entries of [q]x'[q]x in info_fill's order.
USIP_HD void gt_terms(double qx, double qy, double qz, double t[9])
{
    t[0] = qx;
    t[1] = qy;
    t[2] = qz;
    t[3] = qz * qz + qy * qy;           // (4, 4)
    t[4] = qz * qz + qx * qx;           // (5, 5)
    t[5] = qy * qy + qx * qx;           // (6, 6)
    t[6] = qx * qy;                     // -(4, 5)
    t[7] = qx * qz;                     // -(4, 6)
    t[8] = qy * qz;                     // -(5, 6)
}

}  // namespace usip_gt
