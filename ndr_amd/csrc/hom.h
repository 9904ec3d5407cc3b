// Periodic homogenisation of a voxel cell (TPPeriodicHomogenization.hh): what kernels_hom.hip offers to hom.hip.
//
// The unknowns live on the PERIODIC node grid: n[d] nodes per axis (= elements per axis), last axis fastest, node 0 pinned.
// A batch of S strain cases (S = 3 in 2-D, 6 in 3-D) is stored as W[s][node][component].  Element e owns the 2^N nodes
// (e_d + mu_d) mod n[d]; its local node index has axis 0 as the most significant bit, its dof is N * node + component.
#pragma once
#include "vfem_internal.h"

#include <functional>

namespace vfem {

// a periodic node grid: the cell, or a coarse level of its multigrid hierarchy (hom_mg.h)
struct HomGrid {
    int N, S;                // dimension, strain cases
    int n[3];                // periodic nodes (= elements of the cell) per axis; n[2] = 1 in 2-D
    int pn;                  // periodic nodes
};

struct HomProblem : HomGrid {
    int ke;                  // dofs of an element
    const double *K0;        // device, ke x ke: full-density element matrix
    const double *L;         // device, ke x S: L[:, q] = element load of the constant stress C : e_q
    const double *D;         // device, S x S: flattened tensor
    const double *stencil;   // device, 3^N x 2^N x N x N: hom_build_stencil
    double vol;              // voxel volume
    const double *E;         // device, pn: element moduli
};

// per-column scalars of the batched PCG, held in device memory
struct HomState {
    double rz[6], alpha[6], beta[6], bb[6], rr[6];
    int active[6], iters[6];
};

// The apply's table: for neighbour offset o (digits 0, 1, 2 = -1, 0, +1 per axis, axis 0 most significant) and incident element
// a (the element in which the thread's node is local node a: one step back along every axis whose bit is set),
// stencil[o][a] = K0[(a, .), (m, .)] with m the neighbour's local node in that element, or zero when the element does not
// reach the offset.  Per axis: offset -1 needs own position 1 (partner 0), offset +1 own position 0 (partner 1), offset 0 either.
inline void hom_build_stencil(int N, const double *K0, double *stencil) {
    const int npe = 1 << N, ke = N * npe, noff = N == 2 ? 9 : 27;
    for (int o = 0; o < noff; ++o)
        for (int a = 0; a < npe; ++a) {
            int m = 0, v = o;
            bool reach = true;
            for (int d = N - 1; d >= 0; --d, v /= 3) {
                const int od = v % 3, ad = (a >> (N - 1 - d)) & 1;
                if ((od == 0 && ad != 1) || (od == 2 && ad != 0)) reach = false;
                m |= (od == 1 ? ad : (od == 2 ? 1 : 0)) << (N - 1 - d);
            }
            for (int i = 0; i < N; ++i)
                for (int j = 0; j < N; ++j)
                    stencil[((o * npe + a) * N + i) * N + j] = reach ? K0[(a * N + i) * ke + m * N + j] : 0.0;
        }
}

// the checked arguments every vfem_hom_* entry point starts with, the element tables on the device (hom.hip)
struct HomCall {
    HomProblem p;
    DevBuf<double> tables;          // K0 | L | D | stencil
};
void hom_setup(HomCall &c, const char *who, int dim, const int64_t *nelems, const double *K0, const double *L, const double *D,
               double vol, const double *E, hipStream_t s);

constexpr int HOM_THREADS = 256;
inline int hom_node_blocks(const HomGrid &g) { return (g.pn + HOM_THREADS - 1) / HOM_THREADS; }
// the tensor reduction walks the elements with a grid of fixed size (a function of the cell alone: the summation order is fixed)
inline int hom_tensor_blocks(const HomProblem &p) { const int b = hom_node_blocks(p); return b < 512 ? b : 512; }

// out[s] = K_per w[s] (pin row and column = identity); partial (may be null): [S][node blocks] block sums of w[s] . out[s]
void launch_hom_apply(const HomProblem &p, const double *w, double *out, double *partial, hipStream_t s);
// Minv[node] = inverse of the node's N x N diagonal block (identity at the pin), row-major
void launch_hom_jacobi(const HomProblem &p, double *Minv, hipStream_t s);
// b[s][node] = - sum over the incident elements of E_e L[(local node, .), s]; zero at the pin
void launch_hom_rhs(const HomProblem &p, double *b, hipStream_t s);
// alpha[s] = rz[s] / (p . Ap)[s] for the columns still active (0 for a frozen one), from the apply's block sums
void launch_hom_finish_alpha(const HomGrid &g, const double *partial, HomState *st, hipStream_t s);
// x += alpha p, r -= alpha Ap, z = Minv r; partial: [2 S][node blocks] block sums of r . z and r . r
void launch_hom_update(const HomProblem &p, const double *Minv, const double *pv, const double *Ap, double *x, double *r, double *z,
                       const HomState *st, double *partial, hipStream_t s);
// beta[s] = rz_new / rz, rz = rz_new, rr[s]; a column with rr <= tol^2 bb is frozen.  init: rz, bb from the first residual
void launch_hom_finish_beta(const HomGrid &g, const double *partial, HomState *st, double tol, int init, hipStream_t s);
// p = z + beta p
void launch_hom_direction(const HomGrid &g, const double *z, double *pv, const HomState *st, hipStream_t s);
// Eh[q][r] = inv_cell sum_e E_e (w_{q,e} . L[:, r] + vol D[q][r]); partial: S S hom_tensor_blocks doubles, Eh: device S S
void launch_hom_tensor(const HomProblem &p, const double *W, double inv_cell, double *partial, double *Eh, hipStream_t s);
// G[e][q][r] = dE[e] (1 when null) inv_cell (w_q^T K0 w_r + w_q . L[:, r] + L[:, q] . w_r + vol D[q][r]), upper triangle mirrored
void launch_hom_gradient(const HomProblem &p, const double *W, const double *dE, double inv_cell, double *G, hipStream_t s);
// g[e] = sum_{q <= r} wt[q][r] G[e][q][r] with the G of launch_hom_gradient, which is not formed; wt: device S S, read where q <= r
void launch_hom_gradient_contract(const HomProblem &p, const double *W, const double *dE, double inv_cell, const double *wt, double *g,
                                  hipStream_t s);

// The batched PCG of the cell problems (hom.hip), written once for its preconditioners.  It owns the work vectors, the right-hand
// side, the per-column scalars, the read-backs and the error; a preconditioner is the one step that differs:
//   x += alpha p, r -= alpha Ap (not when `first`: x = 0, r = b), z = M^-1 r, partial = [2 S][node blocks] block sums of r . z and r . r
// `exact`: M^-1 is the inverse, so the norms are also read back after the first iteration
struct HomPcgVectors {
    double *x, *r, *z, *pv, *Ap, *partial;
    HomState *st;
};
struct HomPreconditioner {
    std::function<void(bool first, const HomPcgVectors &v)> step;
    bool exact;
};
// W = the S solutions to |r| / |b| <= tol; throws `who`: no convergence ... after max_iter iterations, or `who`: breakdown ... when
// every column froze and one is short of the tolerance (r . z not positive or NaN: a singular cell); the outputs are set first
void hom_pcg(const HomProblem &p, const char *who, const HomPreconditioner &M, double *W, double tol, int max_iter,
             int *iterations_out_host, double *relres_out_host, hipStream_t s);

}  // namespace vfem
