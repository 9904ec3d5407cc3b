// Heat conduction on a degree-1 grid, steady and transient: what kernels_thermal.hip offers to thermal.hip
// and thermal_mg.hip.
//
// The unknown is one temperature per node.  Nodes and elements are numbered as in modal.h (cell_threads.h: last axis fastest, the
// local node index of an element has axis 0 as its most significant bit).  The operator has one form with one or two terms,
//   A = P (sum_e kappa[e] K + sum_e cap[e] M(mb)) P + iota (I - P),
// K a 2^N x 2^N element matrix, M(mb) the capacity matrix of a voxel, which depends only on the number d of axes along which two
// local nodes differ, M[a][b] = mb[popcount(a xor b)], and so travels as dim + 1 doubles; P zeroes the nodes whose byte of `fixed` is
// not 0 (fixed may be null: P = I).  The steady operator is the one-term form: no capacity term (cap null), K = Kc0 the conductivity
// matrix of a full-density voxel and iota = 1, a fixed node's row and column being the identity.  The transient calls fold the
// scalars of the time scheme into K and mb on the host: K = theta Kc0, mb = m / dt for the system operator of a step,
// K = -(1 - theta) Kc0, mb = m / dt and iota = 0 for its right-hand side.  Both forms are instantiations of the same kernels.
#pragma once
#include "modal.h"

#include <functional>
#include <string>

namespace vfem {

constexpr int THERMAL_MAX_COLS = 8;
constexpr int THERMAL_MAX_NPE = 8;          // 2^N for N = 3

struct ThermalMatrix { double k[THERMAL_MAX_NPE * THERMAL_MAX_NPE]; };      // Kc0, row-major 2^N x 2^N: 64 doubles in the kernel arguments
struct ThermalCoef { double c[THERMAL_MAX_COLS]; };
// the capacity matrix of the two-term operator: m[d], d = 0 .. N, the entry for two local nodes that differ along d axes
struct ThermalCapacity { double m[4]; };
struct ThermalTensor { double k[9]; };                                      // the conductivity tensor, row-major N x N

// the operator as the host describes it to a launcher, which picks the one-term or the two-term instantiation by cap
struct ThermalOp {
    ThermalMatrix K;
    const double *kappa;
    ThermalCapacity mb;             // read only with cap
    const double *cap;              // null: the one-term form
};

// Y_c = A X_c, c < ncols: one thread per node forms its 3^N couplings once for all columns.  With b ([column][node]):
// Y_c = A X_c + P b_c, or (residual) Y_c = b_c - A X_c with b as it is.  The one-term instantiation has iota = 1 and b for a residual
// compiled in: anything else is refused
void launch_thermal_apply(const ModalGrid &g, const ThermalOp &op, const uint8_t *fixed, int identity, int ncols, const double *X,
                          const double *b, int residual, double *Y, hipStream_t s);
// d = diag A with iota = 1, or its reciprocal (invert)
void launch_thermal_diagonal(const ModalGrid &g, const ThermalOp &op, const uint8_t *fixed, int invert, double *d, hipStream_t s);
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
// the lower band of A, iota = 1, in the tile layout of vfem_band_spd_factor (n = nodes, w = the sum of the node strides): every
// stored entry of the nb (bt + 1) tiles is written
void launch_thermal_band_assemble(const ModalGrid &g, const ThermalOp &op, const uint8_t *fixed, double *band, hipStream_t s);
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

// Host code of thermal.hip that thermal_mg.hip and transient.hip use too.  The element matrix and the capacity entries [dim + 1] of
// an entry point, after its grid (grid_args.h; w: the entry point's name for the message): there and finite
ThermalMatrix thermal_element_matrix(const std::string &w, int dim, const double *Kc0_host);
ThermalCapacity thermal_capacity_entries(const std::string &w, int dim, const double *m_host);
// The operator of an entry point, the one checker of both forms: the element matrix, with two_term the capacity entries, then the
// element fields (null is refused)
ThermalOp thermal_operator_args(const std::string &w, int dim, const double *K_host, bool two_term, const double *mb_host,
                                const double *kappa, const double *cap);
// what makes the operator singular, for the breakdown messages
inline const char *thermal_singular_because(const ThermalOp &op) {
    return op.cap ? "a free node whose incident elements all have zero conductivity and zero capacity"
                  : "no fixed node, a free node whose incident elements all have zero conductivity";
}
// The PCG loop of vfem_thermal_pcg and vfem_thermal_mg_pcg on A x = b from the x given: z = M^-1 r is the caller's (launched on s);
// the host reads the scalars before the first iteration and then every look_every iterations, stops when |r| / |b| <= tol, and
// throws "not converged after ..." or "breakdown at iteration ..." with the residual.  The outputs are written in every case.
using ThermalPreconditioner = std::function<void(const double *r, double *z)>;
// The operator is a callable (launched on s): out = A v, or with rhs out = rhs - A v; n = nodes, and singular_because words what
// makes this operator singular for the breakdown message.
using ThermalApply = std::function<void(const double *v, const double *rhs, double *out)>;
void thermal_pcg(const std::string &w, long long n, const ThermalApply &apply, const char *singular_because, const double *b, double *x,
                 double tol, int max_iter, int look_every, const ThermalPreconditioner &precondition, int *iterations_out_host,
                 double *relres_out_host, hipStream_t s);

}  // namespace vfem
