// Multigrid preconditioner of the scalar heat operator: what kernels_thermal_mg.hip offers to thermal_mg.hip.
//
// Level 0 is the grid and stays matrix-free from kappa, and from cap in the two-term form (thermal.h; the formulas below name the
// conduction term alone).  Level l + 1 has half the elements per axis; its nodes are the
// even nodes of level l, and a coarse node is fixed exactly when that fine node is.  With I_l the N-linear interpolation and F_l the
// 0/1 diagonal of the free nodes, P_l = F_l I_l F_{l+1},
//   A'_0 = F_0 (sum_e kappa_e Kc0) F_0,    A'_{l+1} = P_l^T A'_l P_l,    A_l = A'_l + (I - F_l).
// A level >= 1 stores A'_l as a 3^N-point stencil, one double per node and offset, node-fastest: A[offset][node].  Offsets are
// numbered as hom_build_stencil numbers them (digits 0, 1, 2 = -1, 0, +1 per axis, axis 0 most significant: neighbour_offset of
// cell_threads.h).  Entries that reach outside the grid or touch a fixed node are zero; the kernels add the identity of the fixed
// nodes themselves.  A level's mask is one byte per node, 0 or 1.  Every kernel is a gather in a fixed order without atomics.
#pragma once
#include "gs_colors.h"
#include "thermal.h"

namespace vfem {

// where a level's couplings come from: the stored stencil A (fine null), or for level 0 the matrix-free operator of thermal.h, in
// its one-term form or (the hierarchy of a transient step) its two-term form sum_e (kappa_e K + cap_e M(mb))
struct ThermalLevelOp {
    const double *A;
    const ThermalOp *fine;          // host; read at the launch
};

// coarse mask: fixed_c[I] = fixed_f[2 I]
void launch_thermal_mg_coarsen_mask(const ModalGrid &fine, const ModalGrid &coarse, const uint8_t *fixed_f, uint8_t *fixed_c, hipStream_t s);
// Ac[O][I] = sum over fine nodes a, b of P[a, I] A'_f[a][b - a] P[b, I + O]: one thread per coarse node and offset
void launch_thermal_mg_galerkin(const ModalGrid &fine, const ModalGrid &coarse, const ThermalLevelOp &src, const uint8_t *fixed_f,
                                const uint8_t *fixed_c, double *Ac, hipStream_t s);
// dinv[node] = 1 / diag A_l of a stored level (1 at a fixed node)
void launch_thermal_mg_dinv(const ModalGrid &g, const double *A, const uint8_t *fixed, double *dinv, hipStream_t s);
// out = A_l x (b null) or b - A_l x on a stored level
void launch_thermal_mg_apply(const ModalGrid &g, const double *A, const uint8_t *fixed, const double *x, const double *b, double *out,
                             hipStream_t s);
// x += dinv (b - A_l x) on the nodes of one colour of for_each_gs_color(N, 1, ...)
void launch_thermal_mg_sweep_colour(const ModalGrid &g, const ThermalLevelOp &src, const uint8_t *fixed, const double *dinv,
                                    const GsColor &colour, double *x, const double *b, hipStream_t s);
// coarse = P^T fine (one thread per coarse node); fine += P coarse (one thread per fine node; fixed fine nodes are not written)
void launch_thermal_mg_restrict(const ModalGrid &fine, const ModalGrid &coarse, const uint8_t *fixed_f, const uint8_t *fixed_c,
                                const double *vf, double *vc, hipStream_t s);
void launch_thermal_mg_prolong_add(const ModalGrid &fine, const ModalGrid &coarse, const uint8_t *fixed_f, const uint8_t *fixed_c,
                                   const double *vc, double *vf, hipStream_t s);
// M (nodes x nodes, zeroed by the caller) = A_l: one thread per row
void launch_thermal_mg_dense(const ModalGrid &g, const ThermalLevelOp &src, const uint8_t *fixed, double *M, hipStream_t s);
// x = b at the fixed nodes (the dense inverse of CoarsestSolver leaves zeros there; A_l has the identity)
void launch_thermal_mg_copy_fixed(long long n, const uint8_t *fixed, const double *b, double *x, hipStream_t s);
// out[i] = in[i] != 0
void launch_thermal_mg_normalise_mask(long long n, const uint8_t *in, uint8_t *out, hipStream_t s);

}  // namespace vfem
