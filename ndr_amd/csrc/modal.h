// Natural frequencies of a degree-1 grid: what kernels_modal.hip offers to modal.hip.
//
// Nodes and elements are numbered with the last axis fastest (cell_threads.h).  A block of vectors is [column][node][dim]: every
// column is a vector of the simulators.  The consistent mass matrix of a unit-density voxel is the tensor product of the 1-D
// h_d / 6 [[2, 1], [1, 2]], the identity across components:  M0[(i, a), (j, b)] = delta_ab prod_d (h_d / 6) (1 + delta(i_d, j_d)).
#pragma once
#include "vfem_internal.h"

namespace vfem {

constexpr int BLOCK_MAX_COLS = 24;      // columns of a block (mass apply, Gram, combine): three blocks of MODAL_MAX_MODES
constexpr int MODAL_MAX_MODES = 8;
constexpr int GRAM_BLOCKS = 1024;       // partials per entry of a Gram matrix: a function of nothing, so the order is fixed
constexpr int GRAM_TILE = 8;            // a thread of the Gram kernel holds at most GRAM_TILE x GRAM_TILE sums
constexpr int COMBINE_TILE = 12;        // output columns of one combine launch: their coefficients travel in the kernel arguments

struct ModalGrid {
    int N;
    int ne[3];              // elements per axis; ne[2] = 1 in 2-D
    double h[3];            // the voxel's edge lengths
    long long nelem, nnode;
};

struct CombineCoef { double c[BLOCK_MAX_COLS][COMBINE_TILE]; };       // c[i][j]: input column i into output column j of the launch
struct ModalCoef { double cK[MODAL_MAX_MODES], cM[MODAL_MAX_MODES]; };

// Y_c = P M(m) P X_c, c < ncols: one thread per node, all columns; mask (may be null): bit a of mask[node] = component a fixed
void launch_modal_mass_apply(const ModalGrid &g, const double *m, const uint8_t *mask, int ncols, const double *X, double *Y,
                             hipStream_t s);
// X_c = P X_c in place
void launch_modal_project(long long nnode, int N, const uint8_t *mask, int ncols, double *X, hipStream_t s);
// G[i][j] = A_i . B_j (row-major, ka x kb, device); partial: GRAM_BLOCKS ka kb doubles
void launch_block_gram(long long n, int ka, const double *A, int kb, const double *B, double *partial, double *G, hipStream_t s);
// B_j = sum_i C[i][j] A_i, i ascending; C: host, kin x kout row-major
void launch_block_combine(long long n, int kin, int kout, const double *A, const double *C, double *B, hipStream_t s);
// g[e] = sum_i (cK[i] dE[e] phi_ie^T K0 phi_ie + cM[i] dm[e] phi_ie^T M0 phi_ie); K0: device, ke x ke
void launch_modal_gradient(const ModalGrid &g, int nmodes, const double *K0, const ModalCoef &c, const double *dE, const double *dm,
                           const double *Phi, double *out, hipStream_t s);

}  // namespace vfem
