// usip_amd/csrc/icp_plane.hip -- the fit of trimmed ICP under the point-to-plane metric on the device:
// pcregrigid's 'Metric' 'pointToPlane' for the refinement of csrc/icp.hip, whose loop launches icp_fit_plane_kernel in
// icp_fit_kernel's place and shares every other launch.  csrc/icp_plane_math.h has the arithmetic, which the host twin
// (csrc/icp_cpu.cpp) shares; include/usip_hip.h (f-28) is the contract; csrc/icp_state.h is what this file and csrc/icp.hip
// share.  No floating-point atomics, no synchronising launch, every index read from memory is clamped.
//
//   icp_fit_plane_kernel   one workgroup of 256 lanes per pair: one lane-strided pass over the kept rows, every lane's 27
//                          partial sums in registers; the tree in three rounds of nine columns over the 20 480-byte LDS array
//                          of icp_fit_kernel (every column is summed alone, so the grouping decides no bit); every lane solves
//                          the 6 x 6 system on the same values and lane 0 writes the sums, the pose, the histories, the state.
#include "icp_state.h"
#include "icp_plane_math.h"

using namespace usip_reg;
using namespace usip_frag;
using namespace usip_icp;
using namespace usip_bank;

namespace {

__global__ __launch_bounds__(LANES) void icp_fit_plane_kernel(Bank bank, Pairs pr, const int32_t* __restrict__ idx,
                                                              const unsigned long long* __restrict__ d2bits,
                                                              const unsigned long long* __restrict__ cut_bits,
                                                              const int32_t* __restrict__ cut_i, double tol_t, double tol_c,
                                                              int32_t* __restrict__ state, double* __restrict__ Rt_all,
                                                              double* __restrict__ hist_all, int32_t* __restrict__ iterations,
                                                              uint8_t* __restrict__ converged, double* __restrict__ fit_sums,
                                                              int max_iterations)
{
    __shared__ double part[LANES][10];
    const int p = blockIdx.x, l = threadIdx.x;
    if (state[p] != RUNNING) return;                                   // workgroup-uniform
    const Range r1 = range_of(bank, pr.frag1, p, pr.Lmax), r2 = range_of(bank, pr.frag2, p, pr.Lmax);
    const int n1 = r1.n, n2 = r2.n, row_len = bank.row_len;            // both >= 1: the state says so
    const unsigned long long cut = cut_bits[p];
    const int icut = cut_i[p];
    const unsigned long long* v = d2bits + (long long)p * pr.Lmax;
    const int32_t* nn = idx + (long long)p * pr.Lmax;
    const float* rows1 = bank.rows + r1.first * row_len;
    const float* rows2 = bank.rows + r2.first * row_len;
    double Rt[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Rt[k] = Rt_all[(long long)p * 12 + k];

    double S[PLANE_SUMS];
#pragma unroll
    for (int k = 0; k < PLANE_SUMS; ++k) S[k] = 0.0;
    for (int i = l; i < n2; i += LANES)
        if (kept(v[i], i, cut, icut)) {
            const float* a = rows1 + (long long)clamp_index(nn[i], n1) * row_len;
            const float* b = rows2 + (long long)i * row_len;
            const double b0 = (double)b[0], b1 = (double)b[1], b2 = (double)b[2];
            plane_terms(S, xform(Rt, 0, b0, b1, b2), xform(Rt, 1, b0, b1, b2), xform(Rt, 2, b0, b1, b2), a);
        }
#pragma unroll
    for (int base = 0; base < PLANE_SUMS; base += 9) {                 // three rounds of nine columns
        if (base) __syncthreads();                                     // every lane has read the round before
#pragma unroll
        for (int k = 0; k < 9; ++k) part[l][k] = S[base + k];
        tree_sum<9>(part, l);
#pragma unroll
        for (int k = 0; k < 9; ++k) S[base + k] = part[0][k];
    }
    double x[6], Rn[12] = {};
    const bool ok = plane_solve(S, x);                                 // every lane: the same instructions on the same values
    if (ok) plane_step(Rt, x, Rn);                                     // (a failed solve's x may hold anything)
    if (l != 0) return;
    if (fit_sums) {                                                    // fit k of the pair goes to slot k - 1
        double* out = fit_sums + ((long long)p * max_iterations + clamp_index(iterations[p], max_iterations)) * PLANE_SUMS;
#pragma unroll
        for (int k = 0; k < PLANE_SUMS; ++k) out[k] = S[k];
    }
    advance(ok, Rn, p, tol_t, tol_c, state, Rt_all, hist_all, iterations, converged);
}

}  // namespace

int usip_icp::launch_fit_plane(const Bank& bank, const Pairs& pr, int P, const int32_t* idx, const unsigned long long* d2bits,
                               const unsigned long long* cut_bits, const int32_t* cut_i, double tol_t, double tol_c,
                               int32_t* state, double* Rt, double* hist, int32_t* iterations, uint8_t* converged,
                               double* fit_sums, int max_iterations, hipStream_t stream)
{
    USIP_LAUNCH(icp_fit_plane_kernel, dim3(P), dim3(LANES), 0, stream, bank, pr, idx, d2bits, cut_bits, cut_i, tol_t, tol_c,
                state, Rt, hist, iterations, converged, fit_sums, max_iterations);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
