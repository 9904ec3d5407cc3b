// Multigrid preconditioner of the periodic cell problems (DESIGN "Periodic homogenisation"): what kernels_hom_mg.hip offers to
// hom_mg.hip.
//
// Level 0 is the cell and stays matrix-free (hom.h).  Level l + 1 has n_d / 2 periodic nodes per axis and stores one N x N block
// per node and neighbour offset, node-fastest: A[offset][i][j][node], 3^N N^2 doubles per node, so that the lanes of a wave load
// neighbouring doubles.  Offsets are numbered as in hom_build_stencil (digits 0, 1, 2 = -1, 0, +1 per axis, axis 0 most
// significant).  The stored operator is the unpinned Galerkin product; the pin (node 0: identity row and column) is applied by the
// kernels that use it.  Vectors of a level are [S][nodes][N].
#pragma once
#include "hom.h"

namespace vfem {

// where a level's blocks come from: the stored array A (E null), or for level 0 hom_build_stencil's table and the moduli
struct HomBlocks {
    const double *A_or_stencil;
    const double *E;
};
// the inverted diagonal blocks: level 0 keeps launch_hom_jacobi's [node][N N], a stored level [N N][node]
struct HomDinv {
    const double *p;
    long long node_stride, entry_stride;
};

// Ac[O][i][j][I] = sum over fine nodes a, b of P[a, I] Af[a][b - a] P[b, I + O], P the periodic N-linear interpolation: one thread
// per coarse node and offset, a gather in fixed order
void launch_hom_mg_galerkin(const HomGrid &fine, const HomGrid &coarse, const HomBlocks &src, double *Ac, hipStream_t s);
// Dinv[i][j][node] = inverse of the node's diagonal block, identity at the pin
void launch_hom_mg_dinv(const HomGrid &g, const double *A, double *Dinv, hipStream_t s);
// out[s] = A_pinned w[s] on a stored level
void launch_hom_mg_apply(const HomGrid &g, const double *A, const double *w, double *out, hipStream_t s);
// out[s] = b[s] - A_pinned x[s]
void launch_hom_mg_residual(const HomGrid &g, const HomBlocks &src, const double *x, const double *b, double *out, hipStream_t s);
// x_node += Dinv_node (b - A_pinned x)_node for the nodes of one colour (the parity of the node index per axis, axis 0 the most
// significant bit); every n_d must be even
void launch_hom_mg_sweep_colour(const HomGrid &g, const HomBlocks &src, const HomDinv &dinv, int colour, double *x, const double *b,
                                hipStream_t s);
// coarse = P^T fine, zero at node 0; fine += P coarse with the coarse value of node 0 counting as zero
void launch_hom_mg_restrict(const HomGrid &fine, const HomGrid &coarse, const double *vf, double *vc, hipStream_t s);
void launch_hom_mg_prolong_add(const HomGrid &fine, const HomGrid &coarse, const double *vc, double *vf, hipStream_t s);
// M (n x n, n = N nodes, zeroed by the caller) += the pinned operator; wrapped neighbours that coincide (2 nodes along an axis) add
void launch_hom_mg_dense(const HomGrid &g, const HomBlocks &src, double *M, hipStream_t s);
// y[s] = Ainv x[s] for all S columns of the level (Ainv: n x n, n = N nodes, full symmetric): the inverse is read once
void launch_hom_mg_gemv(const HomGrid &g, const double *Ainv, const double *x, double *y, hipStream_t s);
// the PCG's vector step without a preconditioner in it: x += alpha p, r -= alpha Ap per column
void launch_hom_mg_update(const HomGrid &g, const double *pv, const double *Ap, double *x, double *r, const HomState *st, hipStream_t s);
// partial: [2 S][node blocks] block sums of r . z and r . r (the layout launch_hom_finish_beta reads)
void launch_hom_mg_dots(const HomGrid &g, const double *r, const double *z, double *partial, hipStream_t s);

}  // namespace vfem
