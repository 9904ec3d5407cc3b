// Method of Moving Asymptotes: what kernels_mma.hip offers to mma.hip.
//
// Per variable j, with xm = max(xmax - xmin, 1e-5) and the gradient g of one of f_0 .. f_m:
//   p = (U - x)^2 (1.001 g+ + 0.001 g- + 1e-5 / xm),   q = (x - L)^2 (0.001 g+ + 1.001 g- + 1e-5 / xm)        (both > 0)
//   alpha = max(xmin, L + 0.1 (x - L), x - move xm),    beta = min(xmax, U - 0.1 (U - x), x + move xm)
//   P = p_0 + sum_i lambda_i p_i,  Q likewise,  x_j(lambda) = clamp((sqrt(P) L + sqrt(Q) U) / (sqrt(P) + sqrt(Q)), alpha, beta)
// Every term is computed without contracted multiply-adds in one written order (tests/mma_cpu.py states the same order), so a term
// is the same double on the device and in numpy and only the order of a sum differs.
#pragma once
#include "vfem_internal.h"

namespace vfem {

constexpr int MMA_MAX_M = 8;
constexpr int MMA_BLOCKS = 1024;        // partials per accumulator: a function of nothing, so the order of a sum is fixed
// accumulators of one dual pass: sum_j psi_j, the m sums G_i, the m (m + 1) / 2 sums H_ik (i <= k)
constexpr int mma_num_acc(int m) { return 1 + m + m * (m + 1) / 2; }

struct MmaProblem {
    long long n;
    int m;
    const double *x, *L, *U, *xmin, *xmax, *g0, *g;        // device; g is [m][n]
    double move;
};

// L, U in place (iter: 1-based number of the step being taken; xold1, xold2 are read from the third step on)
void launch_mma_asymptotes(long long n, int iter, const double *x, const double *xold1, const double *xold2, const double *xmin,
                           const double *xmax, double asyinit, double asyincr, double asydecr, double *L, double *U, hipStream_t s);
// out[0] = sum_j P/(U - x_j) + Q/(x_j - L), out[1 + i] = G_i = sum_j p_ij/(U - x_j) + q_ij/(x_j - L), then the upper triangle of
// H_ik = sum over the j strictly inside (alpha, beta) of h_ij h_kj / psi''_j, row by row; x_j = x_j(lambda), or the current x
// where at_x (then G_i - f_i = b_i).  partial: mma_num_acc(m) * MMA_BLOCKS doubles; out: mma_num_acc(m) doubles (device)
void launch_mma_dual(const MmaProblem &p, const double *lambda_host, int at_x, double *partial, double *out, hipStream_t s);
// xnew[j] = x_j(lambda)
void launch_mma_primal(const MmaProblem &p, const double *lambda_host, double *xnew, hipStream_t s);

}  // namespace vfem
