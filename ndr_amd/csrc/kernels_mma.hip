// Method of Moving Asymptotes on the device: the asymptote update, the fused dual pass and the primal update.
// Everything of size n is elementwise or a sum; the design vector, the asymptotes and the m + 1 gradients are read once per pass
// and p, q, alpha, beta are recomputed in registers.
#include "mma.h"
#include "device_utils.h"

// the terms of the sums are compared with a numpy restatement term by term: no contracted multiply-adds in this file
#pragma clang fp contract(off)

namespace vfem {

static inline unsigned grid_for(long long n, int block, int cap = 4096) {
    long long g = (n + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned) g;
}
static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// two consecutive doubles: one 16-byte access where the arrays are 16-byte aligned, otherwise two 8-byte accesses to the same
// elements, so the partition and the order of a sum do not depend on the alignment (as the PCG vector kernels do)
template <bool VEC>
__device__ __forceinline__ void mma_load2(const double *p, long long i, double &x0, double &x1) {
    if (VEC) { const double2 v = *reinterpret_cast<const double2 *>(p + i); x0 = v.x; x1 = v.y; }
    else { x0 = p[i]; x1 = p[i + 1]; }
}

template <int M> struct MmaLambda { double v[M]; };

// what one variable contributes: its bounds, the coefficients of the m + 1 approximations and their lambda-weighted sums
template <int M> struct MmaVar {
    double L, U, alpha, beta, P, Q, p[M], q[M];
};

__device__ __forceinline__ void mma_pq(double ux2, double xl2, double e, double g, double &p, double &q) {
    const double gp = fmax(g, 0.0), gm = fmax(-g, 0.0);
    p = ux2 * ((1.001 * gp + 0.001 * gm) + e);
    q = xl2 * ((0.001 * gp + 1.001 * gm) + e);
}

template <int M>
__device__ __forceinline__ void mma_var(double x, double L, double U, double xmin, double xmax, double g0, const double (&g)[M],
                                        double move, const MmaLambda<M> &lam, MmaVar<M> &v) {
    const double xm = fmax(xmax - xmin, 1e-5), e = 1e-5 / xm;
    const double ux = U - x, xl = x - L, ux2 = ux * ux, xl2 = xl * xl;
    v.L = L;
    v.U = U;
    v.alpha = fmax(fmax(xmin, L + 0.1 * xl), x - move * xm);
    v.beta = fmin(fmin(xmax, U - 0.1 * ux), x + move * xm);
    mma_pq(ux2, xl2, e, g0, v.P, v.Q);
#pragma unroll
    for (int i = 0; i < M; ++i) {
        mma_pq(ux2, xl2, e, g[i], v.p[i], v.q[i]);
        v.P = v.P + lam.v[i] * v.p[i];
        v.Q = v.Q + lam.v[i] * v.q[i];
    }
}

// the minimiser of P / (U - x) + Q / (x - L) over [alpha, beta]
template <int M>
__device__ __forceinline__ double mma_minimiser(const MmaVar<M> &v) {
    const double sP = sqrt(v.P), sQ = sqrt(v.Q);
    const double xs = (sP * v.L + sQ * v.U) / (sP + sQ);
    return fmin(fmax(xs, v.alpha), v.beta);
}

template <int M, bool AT_X>
__device__ __forceinline__ void mma_accumulate(double x, double L, double U, double xmin, double xmax, double g0, const double (&g)[M],
                                               double move, const MmaLambda<M> &lam, double (&acc)[mma_num_acc(M)]) {
    MmaVar<M> v;
    mma_var<M>(x, L, U, xmin, xmax, g0, g, move, lam, v);
    const double xj = AT_X ? x : mma_minimiser<M>(v);
    const double rU = 1.0 / (U - xj), rL = 1.0 / (xj - L);
    acc[0] += v.P * rU + v.Q * rL;
#pragma unroll
    for (int i = 0; i < M; ++i) acc[1 + i] += v.p[i] * rU + v.q[i] * rL;
    if (!AT_X && xj > v.alpha && xj < v.beta) {
        const double rU2 = rU * rU, rL2 = rL * rL;
        const double w = 1.0 / (2.0 * (v.P * (rU2 * rU) + v.Q * (rL2 * rL)));
        double h[M];
#pragma unroll
        for (int i = 0; i < M; ++i) h[i] = v.p[i] * rU2 - v.q[i] * rL2;
        int a = 1 + M;
#pragma unroll
        for (int i = 0; i < M; ++i) {
            const double hw = h[i] * w;
#pragma unroll
            for (int k = i; k < M; ++k) acc[a++] += hw * h[k];
        }
    }
}

// 1024 blocks, each thread two consecutive variables per step (an odd last variable goes to the first thread after its pairs),
// per-wave shuffle sums, the four waves of a block added in order: partial[a * MMA_BLOCKS + block].  This is block_sum_256 for
// all accumulators behind one barrier (sh[4][NA]) instead of one barrier each.
template <int M, bool AT_X, bool VEC>
__global__ void __launch_bounds__(256, 2) k_mma_dual(long long n, const double *__restrict__ x, const double *__restrict__ L,
                                                     const double *__restrict__ U, const double *__restrict__ xmin,
                                                     const double *__restrict__ xmax, const double *__restrict__ g0,
                                                     const double *__restrict__ g, double move, MmaLambda<M> lam,
                                                     double *__restrict__ partial) {
    constexpr int NA = mma_num_acc(M);
    __shared__ double sh[4][NA];
    double acc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] = 0.0;
    const long long t0 = (long long) blockIdx.x * blockDim.x + threadIdx.x, nt = (long long) gridDim.x * blockDim.x;
    for (long long i = 2 * t0; i + 1 < n; i += 2 * nt) {
        double x0, x1, L0, L1, U0, U1, a0, a1, b0, b1, c0, c1, ga[M], gb[M];
        mma_load2<VEC>(x, i, x0, x1); mma_load2<VEC>(L, i, L0, L1); mma_load2<VEC>(U, i, U0, U1);
        mma_load2<VEC>(xmin, i, a0, a1); mma_load2<VEC>(xmax, i, b0, b1); mma_load2<VEC>(g0, i, c0, c1);
#pragma unroll
        for (int k = 0; k < M; ++k) mma_load2<VEC>(g + (long long) k * n, i, ga[k], gb[k]);
        mma_accumulate<M, AT_X>(x0, L0, U0, a0, b0, c0, ga, move, lam, acc);
        mma_accumulate<M, AT_X>(x1, L1, U1, a1, b1, c1, gb, move, lam, acc);
    }
    if ((n & 1) && t0 == 0) {
        const long long i = n - 1;
        double ga[M];
#pragma unroll
        for (int k = 0; k < M; ++k) ga[k] = g[(long long) k * n + i];
        mma_accumulate<M, AT_X>(x[i], L[i], U[i], xmin[i], xmax[i], g0[i], ga, move, lam, acc);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const double t = wave_sum(acc[a]);
        if (lane == 0) sh[w][a] = t;
    }
    __syncthreads();
    if (threadIdx.x < NA) {
        const int a = threadIdx.x;
        partial[(long long) a * MMA_BLOCKS + blockIdx.x] = sh[0][a] + sh[1][a] + sh[2][a] + sh[3][a];
    }
}

// one finishing block per accumulator
__global__ void __launch_bounds__(256) k_mma_final(const double *__restrict__ partial, double *__restrict__ out) {
    __shared__ double sh[4];
    const double *p = partial + (long long) blockIdx.x * MMA_BLOCKS;
    double acc = 0.0;
    for (int i = threadIdx.x; i < MMA_BLOCKS; i += 256) acc += p[i];
    const double t = block_sum_256(acc, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}

template <int M>
__global__ void __launch_bounds__(256) k_mma_primal(long long n, const double *__restrict__ x, const double *__restrict__ L,
                                                    const double *__restrict__ U, const double *__restrict__ xmin,
                                                    const double *__restrict__ xmax, const double *__restrict__ g0,
                                                    const double *__restrict__ g, double move, MmaLambda<M> lam,
                                                    double *__restrict__ xnew) {
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x) {
        double gi[M];
#pragma unroll
        for (int k = 0; k < M; ++k) gi[k] = g[(long long) k * n + i];
        MmaVar<M> v;
        mma_var<M>(x[i], L[i], U[i], xmin[i], xmax[i], g0[i], gi, move, lam, v);
        xnew[i] = mma_minimiser<M>(v);
    }
}

// iterations 1 and 2: L, U = x -+ asyinit xm.  Later: the distance to the previous point grows by asyincr where the variable kept
// its direction, shrinks by asydecr where it turned, and stays within [0.01 xm, 10 xm] of x
__global__ void __launch_bounds__(256) k_mma_asymptotes(long long n, int iter, const double *__restrict__ x,
                                                        const double *__restrict__ xold1, const double *__restrict__ xold2,
                                                        const double *__restrict__ xmin, const double *__restrict__ xmax,
                                                        double asyinit, double asyincr, double asydecr, double *__restrict__ L,
                                                        double *__restrict__ U) {
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x) {
        const double xi = x[i], xm = fmax(xmax[i] - xmin[i], 1e-5);
        double l, u;
        if (iter <= 2) {
            l = xi - asyinit * xm;
            u = xi + asyinit * xm;
        } else {
            const double x1 = xold1[i], s = (xi - x1) * (x1 - xold2[i]);
            const double f = s > 0.0 ? asyincr : (s < 0.0 ? asydecr : 1.0);
            l = xi - f * (x1 - L[i]);
            u = xi + f * (U[i] - x1);
            l = fmin(fmax(l, xi - 10.0 * xm), xi - 0.01 * xm);
            u = fmax(fmin(u, xi + 10.0 * xm), xi + 0.01 * xm);
        }
        L[i] = l;
        U[i] = u;
    }
}

void launch_mma_asymptotes(long long n, int iter, const double *x, const double *xold1, const double *xold2, const double *xmin,
                           const double *xmax, double asyinit, double asyincr, double asydecr, double *L, double *U, hipStream_t s) {
    k_mma_asymptotes<<<grid_for(n, 256), 256, 0, s>>>(n, iter, x, xold1, xold2, xmin, xmax, asyinit, asyincr, asydecr, L, U);
    VFEM_HIP(hipGetLastError());
}

template <int M>
static void dual_m(const MmaProblem &p, const double *lambda, int at_x, double *partial, double *out, hipStream_t s) {
    MmaLambda<M> lam;
    for (int i = 0; i < M; ++i) lam.v[i] = lambda[i];
    bool vec = aligned16(p.x) && aligned16(p.L) && aligned16(p.U) && aligned16(p.xmin) && aligned16(p.xmax) && aligned16(p.g0);
    for (int i = 0; i < M; ++i) vec = vec && aligned16(p.g + (long long) i * p.n);
#define VFEM_MMA_DUAL(AT_X, VEC)                                                                                                   \
    k_mma_dual<M, AT_X, VEC><<<MMA_BLOCKS, 256, 0, s>>>(p.n, p.x, p.L, p.U, p.xmin, p.xmax, p.g0, p.g, p.move, lam, partial)
    if (at_x) { if (vec) VFEM_MMA_DUAL(true, true); else VFEM_MMA_DUAL(true, false); }
    else { if (vec) VFEM_MMA_DUAL(false, true); else VFEM_MMA_DUAL(false, false); }
#undef VFEM_MMA_DUAL
    k_mma_final<<<mma_num_acc(M), 256, 0, s>>>(partial, out);
    VFEM_HIP(hipGetLastError());
}

template <int M>
static void primal_m(const MmaProblem &p, const double *lambda, double *xnew, hipStream_t s) {
    MmaLambda<M> lam;
    for (int i = 0; i < M; ++i) lam.v[i] = lambda[i];
    k_mma_primal<M><<<grid_for(p.n, 256), 256, 0, s>>>(p.n, p.x, p.L, p.U, p.xmin, p.xmax, p.g0, p.g, p.move, lam, xnew);
    VFEM_HIP(hipGetLastError());
}

void launch_mma_dual(const MmaProblem &p, const double *lambda, int at_x, double *partial, double *out, hipStream_t s) {
    switch (p.m) {
        case 1: return dual_m<1>(p, lambda, at_x, partial, out, s);
        case 2: return dual_m<2>(p, lambda, at_x, partial, out, s);
        case 3: return dual_m<3>(p, lambda, at_x, partial, out, s);
        case 4: return dual_m<4>(p, lambda, at_x, partial, out, s);
        case 5: return dual_m<5>(p, lambda, at_x, partial, out, s);
        case 6: return dual_m<6>(p, lambda, at_x, partial, out, s);
        case 7: return dual_m<7>(p, lambda, at_x, partial, out, s);
        case 8: return dual_m<8>(p, lambda, at_x, partial, out, s);
    }
    throw Error("MMA kernels take 1 to 8 constraints");
}

void launch_mma_primal(const MmaProblem &p, const double *lambda, double *xnew, hipStream_t s) {
    switch (p.m) {
        case 1: return primal_m<1>(p, lambda, xnew, s);
        case 2: return primal_m<2>(p, lambda, xnew, s);
        case 3: return primal_m<3>(p, lambda, xnew, s);
        case 4: return primal_m<4>(p, lambda, xnew, s);
        case 5: return primal_m<5>(p, lambda, xnew, s);
        case 6: return primal_m<6>(p, lambda, xnew, s);
        case 7: return primal_m<7>(p, lambda, xnew, s);
        case 8: return primal_m<8>(p, lambda, xnew, s);
    }
    throw Error("MMA kernels take 1 to 8 constraints");
}

}  // namespace vfem
