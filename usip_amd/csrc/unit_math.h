// usip_amd/csrc/unit_math.h -- the unit normalisation over channels that ends the indoor descriptor head (the
// reference's networks.py:477, d / (|d| + 1e-5)): the arithmetic the device kernels (csrc/unit_columns.hip) and the host twin
// (csrc/unit_columns_cpu.cpp) share, so both round alike.  include/usip_hip.h, section f-25, is the contract.
//
//   x f32 [B][C][M]; a COLUMN is the C values x[b][.][m] of one position, C * M elements apart.
//   forward     s = sum_c (double)x_c * (double)x_c, ascending c from 0 (a product of two float32 values is exact in
//               float64, so contraction cannot change it); n = (float)sqrt(s); t = n + eps in float32; out_c = x_c / t in
//               float32.  One rounding per operation, nothing else.
//   backward    dot = sum_c (double)g_c * (double)x_c, ascending c from 0; with T = (double)t, N = (double)n:
//               dx_c = (float)(g_c / T - (x_c * dot) / ((N * T) * T)), and (float)(g_c / T) where n == 0 -- torch's zero
//               sub-gradient of the norm at the origin.
//   NaN and Inf take no special path: a NaN in a column makes its n, its outputs and its gradients NaN, no other column's.
#pragma once
#include <cmath>
#include <stdint.h>

#ifndef USIP_HD
#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define USIP_HD __host__ __device__ __forceinline__
#else
#define USIP_HD inline
#endif
#endif

namespace usip_unit {

// B, C, M >= 0 and eps >= 0 (a NaN eps fails the comparison); B * M == 0 is a valid call that does nothing
USIP_HD bool bad_dims(int B, int C, int M, float eps) { return B < 0 || C < 0 || M < 0 || !(eps >= 0.f); }

USIP_HD double add_square(double s, float x)
{
    const double v = (double)x;
    return s + v * v;
}

USIP_HD double add_product(double s, float g, float x) { return s + (double)g * (double)x; }

USIP_HD float norm_of(double s) { return (float)sqrt(s); }

USIP_HD float divisor(float n, float eps) { return n + eps; }

USIP_HD float scaled(float x, float t) { return x / t; }

USIP_HD float grad_of(float g, float x, double dot, float n, float t)
{
    const double T = (double)t, N = (double)n;
    const double direct = (double)g / T;
    if (n == 0.f) return (float)direct;
    return (float)(direct - ((double)x * dot) / ((N * T) * T));
}

}  // namespace usip_unit
