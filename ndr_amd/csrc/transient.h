// Transient heat conduction on a degree-1 grid: what kernels_transient.hip offers to transient.hip.
//
// Numbering, the mask and the conductivity term are those of thermal.h.  The capacity matrix of a voxel depends only on the number d
// of axes along which two local nodes differ, M[a][b] = m[popcount(a xor b)], so it travels as dim + 1 doubles.  The two-term
// operator is
//   A(Ka, mb) = P (sum_e kappa[e] Ka + sum_e cap[e] M(mb)) P + iota (I - P),
// with the scalars of the time scheme folded into Ka and mb on the host: Ka = theta Kc0, mb = m / dt for the system operator of a
// step, Ka = -(1 - theta) Kc0, mb = m / dt and iota = 0 for its right-hand side.
#pragma once
#include "thermal.h"

namespace vfem {

// Y_c = A X_c, c < ncols; with b ([column][node]): Y_c = A X_c + P b_c, or (residual) Y_c = b_c - A X_c with b as it is
void launch_transient_apply(const ModalGrid &g, const ThermalMatrix &Ka, const ThermalCapacity &mb, const double *kappa, const double *cap,
                            const uint8_t *fixed, int identity, int ncols, const double *X, const double *b, int residual, double *Y,
                            hipStream_t s);
// d = diag A(Ka, mb) with iota = 1, or its reciprocal (invert)
void launch_transient_diagonal(const ModalGrid &g, const ThermalMatrix &Ka, const ThermalCapacity &mb, const double *kappa,
                               const double *cap, const uint8_t *fixed, int invert, double *d, hipStream_t s);
// the lower band of A(Ka, mb), iota = 1, in the tile layout of vfem_band_spd_factor (thermal_band_geometry): every stored entry of
// the nb (bt + 1) tiles is written
void launch_transient_band_assemble(const ModalGrid &g, const ThermalMatrix &Ka, const ThermalCapacity &mb, const double *kappa,
                                    const double *cap, const uint8_t *fixed, double *band, hipStream_t s);
// out[e] = -sum_{n = 1 .. steps} (dcap[e] / dt lam_e^n . M(m) (T_e^n - T_e^(n-1)) + dkappa[e] lam_e^n . K (theta T_e^n + (1 - theta) T_e^(n-1)))
// over the rows of T and Lam ([steps + 1][node]; row 0 of Lam is not read)
void launch_transient_gradient(const ModalGrid &g, const ThermalMatrix &K, const ThermalCapacity &m, long long steps, double dt,
                               double theta, const double *dkappa, const double *dcap, const double *T, const double *Lam, double *out,
                               hipStream_t s);

}  // namespace vfem
