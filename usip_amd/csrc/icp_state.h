// usip_amd/csrc/icp_state.h -- what the two translation units of the ICP loop share on the device: csrc/icp.hip (the loop
// and the point-to-point fit) and csrc/icp_plane.hip (the point-to-plane fit, f-28).  A pair's state lives in
// device memory between the launches: every workgroup reads it first and leaves when the pair has stopped, a fit's lane 0
// writes it (advance), the host never reads it.
#pragma once
#include "common.h"
#include "bank.h"
#include "icp_math.h"

namespace usip_icp {

struct Pairs {
    const int32_t* frag1;
    const int32_t* frag2;
    int Lmax;
};

__device__ __forceinline__ usip_bank::Range range_of(const usip_bank::Bank& bank, const int32_t* frag, int p, int lmax)
{
    return bank.range(frag[p], lmax);
}

// Lane 0 after a fit.  ok false: the pair ends with the pose it has (rule 4).  Otherwise Rn replaces the pose, the two
// changes enter the histories and the stopping rule is read (rule 5).
__device__ __forceinline__ void advance(bool ok, const double* Rn, int p, double tol_t, double tol_c, int32_t* state,
                                        double* Rt_all, double* hist_all, int32_t* iterations, uint8_t* converged)
{
    double* Rt = Rt_all + (long long)p * 12;
    double* h = hist_all + (long long)p * 6;
    if (!ok) {                                                         // the last finite pose stays
        state[p] = STOPPED;
        return;
    }
    double old[12], dt, dc;
#pragma unroll
    for (int k = 0; k < 12; ++k) old[k] = Rt[k];
    pose_delta(Rn, old, &dt, &dc);
#pragma unroll
    for (int k = 0; k < 12; ++k) Rt[k] = Rn[k];
    push(h, dt);
    push(h + 3, dc);
    const int k = iterations[p] + 1;
    iterations[p] = k;
    if (recent_mean(h, k) <= tol_t && recent_mean(h + 3, k) <= tol_c) {
        converged[p] = 1;
        state[p] = STOPPED;
    }
}

// csrc/icp_plane.hip: icp_fit_plane_kernel in icp_fit_kernel's place of the sequence, one workgroup of LANES per pair;
// the arguments are icp_fit_kernel's (the workspace's arrays) plus fit_sums f64 [P][max_iterations][27] (NULL: not wanted).
// -> USIP_OK or the launch's HIP error.
int launch_fit_plane(const usip_bank::Bank& bank, const Pairs& pr, int P, const int32_t* idx, const unsigned long long* d2bits,
                     const unsigned long long* cut_bits, const int32_t* cut_i, double tol_t, double tol_c, int32_t* state,
                     double* Rt, double* hist, int32_t* iterations, uint8_t* converged, double* fit_sums, int max_iterations,
                     hipStream_t stream);

}  // namespace usip_icp
