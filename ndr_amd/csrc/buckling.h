// Linearised buckling of a degree-1 grid: what kernels_buckling.hip offers to buckling.hip.
//
// Numbering, blocks of vectors and the node mask are those of modal.h.  The consistent geometric stiffness of element e is the same
// scalar matrix on every displacement component, linear in the element's 2^N N displacements:
//   K_G,e[(n, a), (m, b)] = delta_ab mG[e] sum_j u_ej T_j[n][m],   T_j[n][m] = int_e grad N_n^T (C : B_j(x)) grad N_m dV,
// B_j the strain of a unit displacement at dof j.  The table T [2^N N][2^N][2^N] depends on the tensor and the voxel's edge lengths
// only; buckling.hip forms it on the host (2 Gauss points per axis: exact) and the kernels read it by uniform loads.
#pragma once
#include "modal.h"

namespace vfem {

constexpr int BUCKLING_MAX_MODES = MODAL_MAX_MODES;

struct BucklingCoef { double c[BUCKLING_MAX_MODES], cK[BUCKLING_MAX_MODES]; };

inline int buckling_table_size(int N) { return N * (1 << N) * (1 << N) * (1 << N); }

// Y_c = P K_G(mG, u) P X_c, c < ncols: one thread per node forms its 3^N couplings once, then walks the columns; mask may be null
void launch_buckling_geom_apply(const ModalGrid &g, const double *T, const double *mG, const double *u, const uint8_t *mask, int ncols,
                                const double *X, double *Y, hipStream_t s);
// a[(node, a)] = sum_i c[i] d(phi_i^T K_G phi_i)/du: gathered over the elements around the node; 0 where the mask says so
void launch_buckling_adjoint_load(const ModalGrid &g, const double *T, const double *mG, const uint8_t *mask, int nmodes,
                                  const BucklingCoef &c, const double *Phi, double *a, hipStream_t s);
// g[e] = dmG[e] sum_i c[i] sum_j u_ej phi_ie^T T_j phi_ie + dE[e] (sum_i cK[i] phi_ie^T K0 phi_ie - v_e^T K0 u_e); K0: device, ke x ke
void launch_buckling_gradient(const ModalGrid &g, const double *T, const double *K0, int nmodes, const BucklingCoef &c,
                              const double *dmG, const double *dE, const double *u, const double *v, const double *Phi, double *out,
                              hipStream_t s);

}  // namespace vfem
