// Transient heat conduction on a degree-1 grid: what kernels_transient.hip offers to transient.hip.
//
// Numbering, the mask, the two-term operator of a step and its capacity entries are those of thermal.h, whose kernels apply it,
// assemble it and precondition it.  What is the transient problem's alone is the density gradient summed over the steps of a march.
#pragma once
#include "thermal.h"

namespace vfem {

// out[e] = -sum_{n = 1 .. steps} (dcap[e] / dt lam_e^n . M(m) (T_e^n - T_e^(n-1)) + dkappa[e] lam_e^n . K (theta T_e^n + (1 - theta) T_e^(n-1)))
// over the rows of T and Lam ([steps + 1][node]; row 0 of Lam is not read)
void launch_transient_gradient(const ModalGrid &g, const ThermalMatrix &K, const ThermalCapacity &m, long long steps, double dt,
                               double theta, const double *dkappa, const double *dcap, const double *T, const double *Lam, double *out,
                               hipStream_t s);

}  // namespace vfem
