// usip_amd/csrc/pool_order.h -- the order every max-pooling kernel ranks by (group.hip, group_wide.hip).
#pragma once
#include "common.h"

// The pooling order: NaN above everything, then the value; at equal values (two NaNs are equal here) the lower k.
// Inside a lane, where k only grows, pool_gt<true> says whether a later element replaces the best so far.  A lane whose
// best is a NaN then enters the cross-lane steps as (+inf, k - POOL_NAN): the steps' plain rule, ov > best ||
// (ov == best && ok < bk), lets it beat a real +inf, lets the lowest NaN k win, and is the rule rows without NaN always
// had; whoever stores finds bk < 0 and puts k and the NaN back.  NANS = false (values that passed through fmaxf(., 0)
// cannot be NaN) is v > best and nothing else.
constexpr int POOL_NAN = 0x40000000;
template <bool NANS>
__device__ __forceinline__ bool pool_gt(float v, float best)
{
    return NANS ? (!(v <= best) && best == best) : v > best;
}
__device__ __forceinline__ void pool_hide_nan(float& best, int& bk)
{
    if (best != best) { best = __builtin_inff(); bk -= POOL_NAN; }
}
