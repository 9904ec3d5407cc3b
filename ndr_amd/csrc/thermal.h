// Steady heat conduction on a degree-1 grid: what kernels_thermal.hip offers to thermal.hip.
//
// The unknown is one temperature per node.  Nodes and elements are numbered as in modal.h (cell_threads.h: last axis fastest, the
// local node index of an element has axis 0 as its most significant bit).  The operator is
//   A(kappa) = P (sum_e kappa[e] Kc0) P + (I - P),
// Kc0 the 2^N x 2^N conductivity matrix of a full-density voxel, P zeroing the nodes whose byte of `fixed` is not 0 (fixed may be
// null: P = I).  A fixed node's row and column are the identity.
#pragma once
#include "modal.h"

#include <functional>
#include <string>

namespace vfem {

constexpr int THERMAL_MAX_COLS = 8;
constexpr int THERMAL_MAX_NPE = 8;          // 2^N for N = 3

struct ThermalMatrix { double k[THERMAL_MAX_NPE * THERMAL_MAX_NPE]; };      // Kc0, row-major 2^N x 2^N: 64 doubles in the kernel arguments
struct ThermalCoef { double c[THERMAL_MAX_COLS]; };
// the capacity matrix of the transient operator (transient.h): m[d], d = 0 .. N, the entry for two local nodes that differ along d axes
struct ThermalCapacity { double m[4]; };
struct ThermalTensor { double k[9]; };                                      // the conductivity tensor, row-major N x N

// Y_c = A X_c, c < ncols: one thread per node forms its 3^N couplings once for all columns.  With b (ncols = 1): Y = b - A X.
void launch_thermal_apply(const ModalGrid &g, const ThermalMatrix &K, const double *kappa, const uint8_t *fixed, int ncols,
                          const double *X, const double *b, double *Y, hipStream_t s);
// d = diag A, or 1 / diag A (invert)
void launch_thermal_diagonal(const ModalGrid &g, const ThermalMatrix &K, const double *kappa, const uint8_t *fixed, int invert,
                             double *d, hipStream_t s);
// f_out = P (f_in + sum_e q[e] vol / 2^N); f_in or q may be null, f_out may be f_in
void launch_thermal_source(const ModalGrid &g, const double *q, const uint8_t *fixed, const double *f_in, double *f_out,
                           hipStream_t s);
// n = nodes, w = the half-bandwidth of A: the sum of the node strides
inline void thermal_band_geometry(const ModalGrid &g, long long &n, long long &w) {
    n = 1;
    w = 0;
    for (int a = g.N - 1; a >= 0; --a) {
        w += n;
        n *= g.ne[a] + 1;
    }
}
// the lower band of A in the tile layout of vfem_band_spd_factor (n = nodes, w = the sum of the node strides): every stored entry
// of the nb (bt + 1) tiles is written
void launch_thermal_band_assemble(const ModalGrid &g, const ThermalMatrix &K, const double *kappa, const uint8_t *fixed, double *band,
                                  hipStream_t s);
// g[e] = dkappa[e] sum_i c[i] a_ie^T Kc0 b_ie over the ncols column pairs of A and B ([column][node]); B may be A
void launch_thermal_gradient(const ModalGrid &g, const ThermalMatrix &K, int ncols, const ThermalCoef &c, const double *dkappa,
                             const double *A, const double *B, double *out, hipStream_t s);
// flux[e][a] = -kappa[e] sum_d k[a][d] (grad T)_d at the element centre
void launch_thermal_flux(const ModalGrid &g, const ThermalTensor &k, const double *kappa, const double *T, double *flux, hipStream_t s);
// z = dinv r (the Jacobi preconditioner)
void launch_thermal_scale(long long n, const double *dinv, const double *r, double *z, hipStream_t s);
// The scalars of the PCG loop live on the device (sc: [0] r.z, [1] the last r.z, [2] p.Ap, [3] r.r, [4] b.b, [5] the iteration at
// which p.Ap stopped being positive (0: none), [6] that p.Ap, [7] r.r then).  Stage 1 (after p.Ap) records a breakdown; from then
// on both stages make the step and the direction update neutral (alpha = 0, beta = 0), so the loop idles until the host looks.
void launch_thermal_pcg_guard(double *sc, int stage, int iteration, hipStream_t s);

// Host code of thermal.hip that thermal_mg.hip uses too.  The element matrix of an entry point, after its grid (grid_args.h; w: the
// entry point's name for the message): there and finite
ThermalMatrix thermal_element_matrix(const std::string &w, int dim, const double *Kc0_host);
// The PCG loop of vfem_thermal_pcg and vfem_thermal_mg_pcg on A x = b from the x given: z = M^-1 r is the caller's (launched on s);
// the host reads the scalars before the first iteration and then every look_every iterations, stops when |r| / |b| <= tol, and
// throws "not converged after ..." or "breakdown at iteration ..." with the residual.  The outputs are written in every case.
using ThermalPreconditioner = std::function<void(const double *r, double *z)>;
// The loop itself takes the operator as a callable (launched on s): out = A v, or with rhs out = rhs - A v; n = nodes, and
// singular_because words what makes this operator singular for the breakdown message.  The form below is the steady operator's;
// transient.hip hands in the two-term operator.
using ThermalApply = std::function<void(const double *v, const double *rhs, double *out)>;
void thermal_pcg(const std::string &w, long long n, const ThermalApply &apply, const char *singular_because, const double *b, double *x,
                 double tol, int max_iter, int look_every, const ThermalPreconditioner &precondition, int *iterations_out_host,
                 double *relres_out_host, hipStream_t s);
void thermal_pcg(const std::string &w, const ModalGrid &g, const ThermalMatrix &K, const double *kappa, const uint8_t *fixed,
                 const double *b, double *x, double tol, int max_iter, int look_every, const ThermalPreconditioner &precondition,
                 int *iterations_out_host, double *relres_out_host, hipStream_t s);

}  // namespace vfem
