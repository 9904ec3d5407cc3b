// Thermo-elastic coupling of a degree-1 grid: what kernels_thermoelastic.hip offers to thermoelastic.hip.
//
// Numbering and the node mask are those of modal.h.  theta = T - T_ref at the nodes is interpolated inside the element: the
// consistent coupling matrix of a full-density voxel,
//   G[(n, a)][m] = int beta_aq dN_n/dx_q N_m dV,   beta = C : alpha,
// has ke = N 2^N rows (dof = N node + component, the local node order of K0) and npe = 2^N columns, row-major; the caller forms
// it.  The thermal load of a case is  f = P sum_e E[e] G theta_e.
#pragma once
#include "modal.h"

namespace vfem {

constexpr int TE_MAX_CASES = 8;
constexpr int TE_MAX_G = 192;           // ke npe = N 4^N for N = 3

struct TeMatrix { double G[TE_MAX_G]; };                                    // one case: in the kernel arguments of the load
struct TeCoef { double a[TE_MAX_CASES], tref[TE_MAX_CASES]; };

// f_out = P (f_in + sum_e E[e] G (T_e - tref)): one thread per node gathers its 2^N elements in ascending local-node order, the
// columns of G ascending within each.  f_in and mask may be null, f_out may be f_in.
void launch_te_load(const ModalGrid &g, const TeMatrix &G, double tref, const double *E, const double *T, const uint8_t *mask,
                    const double *f_in, double *f_out, hipStream_t s);
// q[node] = P_T sum_i a[i] sum_e E[e] (G_i^T u_ie)[node]: the transpose; cases, then elements, then rows (n, a) ascending.
// G: device, [ncases][ke][npe]; U: [case][node][N]; fixed (may be null): one byte per node, nonzero = q is 0 there
void launch_te_adjoint_source(const ModalGrid &g, int ncases, const double *G, const TeCoef &c, const double *E, const double *U,
                              const uint8_t *fixed, double *q, hipStream_t s);
// g_out[e] = g_in[e] + dE[e] sum_i a[i] u_ie^T G_i (T_e - tref[i]); g_in may be null, g_out may be g_in
void launch_te_gradient(const ModalGrid &g, int ncases, const double *G, const TeCoef &c, const double *dE, const double *T,
                        const double *U, const double *g_in, double *g_out, hipStream_t s);

}  // namespace vfem
