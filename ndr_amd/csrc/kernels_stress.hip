// Element stresses of a degree-1 grid (stress.h): the strain / stress / von Mises field, the p-norm measure, its
// adjoint load and its density gradient.
//
// Thread mapping (cell_threads.h): a block is 64 lanes along the last (fastest) axis by 4 rows of the axis before
// it; in 3-D blockIdx.z walks axis 0.  The field and gradient kernels give one thread to an element; the adjoint load is an element
// kernel that stores S doubles per element and a kernel with one thread per NODE, which gathers from its up to 2^N incident elements
// in ascending local-node order: no atomics, bit-identical run to run.  An element's strain comes from the 2^N nodal values of u:
// eps needs only the sums of u over the two faces normal to each axis, so no 6 x 24 matrix is read.  The tensor travels in the kernel
// arguments (StressProblem::Dm).
//
// u (and lambda) may start 8 bytes off a 16-byte line: the 2-D kernels load a node's two components as one 16-byte access only
// where the launcher found the arrays aligned (VEC); a 3-D node is 24 bytes, loaded as three doubles.
#include "stress.h"

#include "cell_threads.h"
#include "device_utils.h"

namespace vfem {

namespace {

template <int N>
struct StressTraits {
    static constexpr int S = N == 2 ? 3 : 6;
    static constexpr int NPE = 1 << N;
    static constexpr int KE = N * NPE;
};

// the N components of the 2^N nodes of element ec
template <int N, bool VEC>
__device__ __forceinline__ void gather_element(const StressProblem &p, const int (&ec)[N], const double *__restrict__ u,
                                               double (&ue)[1 << N][N]) {
#pragma unroll
    for (int m = 0; m < (1 << N); ++m) {
        int c[N];
#pragma unroll
        for (int d = 0; d < N; ++d) c[d] = ec[d] + node_bit<N>(m, d);
        const long long nd = flat_index<N>(p.ne, 1, c);
        if constexpr (N == 2 && VEC) {
            const double2 v = *reinterpret_cast<const double2 *>(u + 2 * nd);
            ue[m][0] = v.x; ue[m][1] = v.y;
        } else {
#pragma unroll
            for (int b = 0; b < N; ++b) ue[m][b] = u[N * nd + b];
        }
    }
}

// eps = Bbar u_e: G[k][j] = d u_j / d x_k from the difference of the sums over the two faces normal to axis k
template <int N>
__device__ __forceinline__ void element_strain(const StressProblem &p, const double (&ue)[1 << N][N], double (&eps)[StressTraits<N>::S]) {
    double G[N][N];
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
        for (int j = 0; j < N; ++j) {
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < (1 << N); ++m) v += node_bit<N>(m, k) ? ue[m][j] : -ue[m][j];
            G[k][j] = v * p.gs[k];
        }
    if constexpr (N == 2) {
        eps[0] = G[0][0]; eps[1] = G[1][1]; eps[2] = 0.5 * (G[0][1] + G[1][0]);
    } else {
        eps[0] = G[0][0]; eps[1] = G[1][1]; eps[2] = G[2][2];
        eps[3] = 0.5 * (G[1][2] + G[2][1]); eps[4] = 0.5 * (G[0][2] + G[2][0]); eps[5] = 0.5 * (G[0][1] + G[1][0]);
    }
}

// s = C : eps (tensor components; Dm has the shear columns doubled)
template <int N>
__device__ __forceinline__ void contract_tensor(const StressProblem &p, const double (&eps)[StressTraits<N>::S],
                                                double (&s)[StressTraits<N>::S]) {
    constexpr int S = StressTraits<N>::S;
#pragma unroll
    for (int q = 0; q < S; ++q) {
        double v = 0.0;
#pragma unroll
        for (int r = 0; r < S; ++r) v = fma(p.Dm[q * S + r], eps[r], v);
        s[q] = v;
    }
}

template <int N>
__device__ __forceinline__ double von_mises(const double (&s)[StressTraits<N>::S]) {
    if constexpr (N == 2) {
        return sqrt(s[0] * s[0] - s[0] * s[1] + s[1] * s[1] + 3.0 * s[2] * s[2]);
    } else {
        const double a = s[0] - s[1], b = s[1] - s[2], c = s[2] - s[0];
        return sqrt(0.5 * (a * a + b * b + c * c) + 3.0 * (s[3] * s[3] + s[4] * s[4] + s[5] * s[5]));
    }
}

// d vm / d s_q for the flattened components (a shear component stands for both of its tensor entries); 0 where vm = 0.  Of degree
// 0 in s: the derivative at m s, m > 0, is the one at s
template <int N>
__device__ __forceinline__ void von_mises_derivative(const double (&s)[StressTraits<N>::S], double vm, double (&dv)[StressTraits<N>::S]) {
    const double r = vm > 0.0 ? 0.5 / vm : 0.0;
    if constexpr (N == 2) {
        dv[0] = (2.0 * s[0] - s[1]) * r; dv[1] = (2.0 * s[1] - s[0]) * r; dv[2] = 6.0 * s[2] * r;
    } else {
        dv[0] = (2.0 * s[0] - s[1] - s[2]) * r; dv[1] = (2.0 * s[1] - s[2] - s[0]) * r; dv[2] = (2.0 * s[2] - s[0] - s[1]) * r;
        dv[3] = 6.0 * s[3] * r; dv[4] = 6.0 * s[4] * r; dv[5] = 6.0 * s[5] * r;
    }
}

// x^(P-1), 0 <= x <= 1: by squaring where P - 1 is a small whole number (ip >= 0; the same for every lane), else pow
__device__ __forceinline__ double weight_power(double x, double pm1, int ip) {
    if (ip >= 0) {
        double r = 1.0, b = x;
        for (int k = ip; k > 0; k >>= 1) {
            if (k & 1) r *= b;
            b *= b;
        }
        return r;
    }
    return pow(x, pm1);
}

template <int N, bool VEC>
__global__ void __launch_bounds__(256) k_stress_fields(StressProblem p, const double *__restrict__ m, const double *__restrict__ u,
                                                       double *__restrict__ strain, double *__restrict__ stress,
                                                       double *__restrict__ vm) {
    constexpr int S = StressTraits<N>::S;
    int ec[N];
    if (!thread_cell<N>(p.ne, 0, ec)) return;
    const long long e = flat_index<N>(p.ne, 0, ec);
    double ue[1 << N][N], eps[S], s[S];
    gather_element<N, VEC>(p, ec, u, ue);
    element_strain<N>(p, ue, eps);
    if (strain) {
#pragma unroll
        for (int q = 0; q < S; ++q) strain[e * S + q] = eps[q];
    }
    if (!stress && !vm) return;
    contract_tensor<N>(p, eps, s);
    const double me = m[e];
#pragma unroll
    for (int q = 0; q < S; ++q) s[q] *= me;
    if (stress) {
#pragma unroll
        for (int q = 0; q < S; ++q) stress[e * S + q] = s[q];
    }
    if (vm) vm[e] = von_mises<N>(s);
}

// ---- the measure: two two-stage reductions, every stage in a fixed order ----

__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }       // a NaN stays

template <bool MAX>
__device__ __forceinline__ double block_reduce_256(double v, double *sh) {          // valid in thread 0
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(v, off, 64);
        v = MAX ? nan_max(v, o) : v + o;
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (MAX) return nan_max(nan_max(nan_max(sh[0], sh[1]), sh[2]), sh[3]);
    return sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ void __launch_bounds__(256) k_stress_max_partial(long long n, const double *__restrict__ vm, double *__restrict__ partial) {
    __shared__ double sh[4];
    double acc = 0.0;
    for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < n; i += (long long) gridDim.x * 256) acc = nan_max(acc, vm[i]);
    const double t = block_reduce_256<true>(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ void __launch_bounds__(256) k_stress_max_finish(int nparts, const double *__restrict__ partial, double *__restrict__ out) {
    __shared__ double sh[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) acc = nan_max(acc, partial[i]);
    const double t = block_reduce_256<true>(acc, sh);
    if (threadIdx.x == 0) out[1] = t;
}

__global__ void __launch_bounds__(256) k_stress_power_partial(long long n, const double *__restrict__ vm, double P,
                                                              const double *__restrict__ out, double *__restrict__ partial) {
    __shared__ double sh[4];
    const double vmax = out[1];
    double acc = 0.0;
    if (vmax != 0.0)
        for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < n; i += (long long) gridDim.x * 256) acc += pow(vm[i] / vmax, P);
    const double t = block_reduce_256<false>(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ void __launch_bounds__(256) k_stress_pnorm_finish(int nparts, const double *__restrict__ partial, double P,
                                                             double *__restrict__ out) {
    __shared__ double sh[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) acc += partial[i];
    const double t = block_reduce_256<false>(acc, sh);
    if (threadIdx.x == 0) {
        const double vmax = out[1];
        out[0] = vmax == 0.0 ? 0.0 : vmax * pow(t, 1.0 / P);
    }
}

// ---- the adjoint load: what each element sends to its nodes (one thread per element), then a gather per node ----
//
// work[e][r] = (vm_e / J)^(P-1) m_e t_r,  t_r = sum_q dv_q Dm[q][r] = d vm / d eps_r at unit multiplier: S doubles per element.  The
// node kernel then needs 2^N S loads and a few products per node.  Measured at 512 x 256 x 256: 1.79 .. 1.81 ms.  Gathering
// straight from u instead, with no scratch, recomputes every element's strain, stress and weight 2^N times from 2^N N loads each:
// 3.52 ms.  The scratch stored component by component (work[r][e], coalesced along a row) measured 1.97 ms.

template <int N, bool VEC>
__global__ void __launch_bounds__(256) k_stress_adjoint_elements(StressProblem p, const double *__restrict__ m, const double *__restrict__ u,
                                                                 double invJ, double pm1, int ip, double *__restrict__ work) {
    constexpr int S = StressTraits<N>::S;
    int ec[N];
    if (!thread_cell<N>(p.ne, 0, ec)) return;
    const long long e = flat_index<N>(p.ne, 0, ec);
    double ue[1 << N][N], eps[S], s[S], dv[S];
    gather_element<N, VEC>(p, ec, u, ue);
    element_strain<N>(p, ue, eps);
    contract_tensor<N>(p, eps, s);
    const double me = m[e];
    const double vm0 = von_mises<N>(s), vm = me * vm0;
    von_mises_derivative<N>(s, vm > 0.0 ? vm0 : 0.0, dv);
    const double coef = weight_power(vm * invJ, pm1, ip) * me;
#pragma unroll
    for (int r = 0; r < S; ++r) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < S; ++q) v = fma(dv[q], p.Dm[q * S + r], v);
        work[e * S + r] = coef * v;
    }
}

template <int N>
__global__ void __launch_bounds__(256) k_stress_adjoint_gather(StressProblem p, const double *__restrict__ work,
                                                               const uint8_t *__restrict__ mask, double *__restrict__ a) {
    constexpr int S = StressTraits<N>::S;
    int c[N];
    if (!thread_cell<N>(p.ne, 1, c)) return;
    const long long node = flat_index<N>(p.ne, 1, c);
    double acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.0;
    // in element `el` this node is local node `el`: the element sits one step back along every axis whose bit is set; ascending order
#pragma unroll
    for (int el = 0; el < (1 << N); ++el) {
        int ec[N];
        bool in = true;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            ec[d] = c[d] - node_bit<N>(el, d);
            in = in && ec[d] >= 0 && ec[d] < p.ne[d];
        }
        if (!in) continue;
        const double *t = work + flat_index<N>(p.ne, 0, ec) * S;
        double g[N];
#pragma unroll
        for (int d = 0; d < N; ++d) g[d] = node_bit<N>(el, d) ? p.gs[d] : -p.gs[d];
        // Bbar_j^T t = T g_j with the symmetric T: t_ii on the diagonal, t_ik / 2 off it
        if constexpr (N == 2) {
            acc[0] += t[0] * g[0] + 0.5 * t[2] * g[1];
            acc[1] += 0.5 * t[2] * g[0] + t[1] * g[1];
        } else {
            acc[0] += t[0] * g[0] + 0.5 * (t[5] * g[1] + t[4] * g[2]);
            acc[1] += t[1] * g[1] + 0.5 * (t[5] * g[0] + t[3] * g[2]);
            acc[2] += t[2] * g[2] + 0.5 * (t[4] * g[0] + t[3] * g[1]);
        }
    }
    const int fixed = mask ? mask[node] : 0;
#pragma unroll
    for (int j = 0; j < N; ++j) a[N * node + j] = ((fixed >> j) & 1) ? 0.0 : acc[j];
}

// ---- the density gradient: the two-field form of k_compliance_gradient with the explicit term ----

template <int N, bool VEC>
__global__ void __launch_bounds__(256) k_stress_gradient(StressProblem p, const double *__restrict__ K0, const double *__restrict__ m,
                                                         const double *__restrict__ dm, const double *__restrict__ dE,
                                                         const double *__restrict__ u, const double *__restrict__ lambda, double invJ,
                                                         double pm1, int ip, double *__restrict__ g) {
    constexpr int S = StressTraits<N>::S, NPE = StressTraits<N>::NPE, KE = StressTraits<N>::KE;
    int ec[N];
    if (!thread_cell<N>(p.ne, 0, ec)) return;
    const long long e = flat_index<N>(p.ne, 0, ec);
    double ue[NPE][N], eps[S], s[S];
    gather_element<N, VEC>(p, ec, u, ue);
    // lambda_e^T K0 u_e, one node's rows at a time.  Rolled: lambda's values and the rows of K0 are not all in flight at once, 67
    // registers instead of the 171 of the unrolled double loop, which measured 3.13 ms against 1.00 .. 1.04 ms (512 x 256 x 256)
    double en = 0.0;
#pragma unroll 1
    for (int mn = 0; mn < NPE; ++mn) {
        int c[N];
#pragma unroll
        for (int d = 0; d < N; ++d) c[d] = ec[d] + node_bit<N>(mn, d);
        const long long nd = flat_index<N>(p.ne, 1, c);
        double le[N];
        if constexpr (N == 2 && VEC) {
            const double2 v = *reinterpret_cast<const double2 *>(lambda + 2 * nd);
            le[0] = v.x; le[1] = v.y;
        } else {
#pragma unroll
            for (int b = 0; b < N; ++b) le[b] = lambda[N * nd + b];
        }
        const double *rows = K0 + (long long) mn * N * KE;
#pragma unroll
        for (int b = 0; b < N; ++b) {
            double acc = 0.0;
#pragma unroll
            for (int c2 = 0; c2 < KE; ++c2) acc = fma(rows[b * KE + c2], ue[c2 / N][c2 % N], acc);
            en = fma(le[b], acc, en);
        }
    }
    element_strain<N>(p, ue, eps);
    contract_tensor<N>(p, eps, s);
    const double vm0 = von_mises<N>(s);                            // vm_e / m_e
    const double w = weight_power(m[e] * vm0 * invJ, pm1, ip);
    g[e] = w * dm[e] * vm0 - dE[e] * en;
}

dim3 cell_grid(const StressProblem &p, int extra) { return vfem::cell_grid(p.N, p.ne, extra); }

bool aligned16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

// whole-number exponent of weight_power, or -1
int whole_exponent(double pm1) { return pm1 >= 0.0 && pm1 <= 1024.0 && pm1 == (double) (int) pm1 ? (int) pm1 : -1; }

const dim3 STRESS_BLOCK = cell_block();

}  // namespace

void launch_stress_fields(const StressProblem &p, const double *m, const double *u, double *strain, double *stress, double *vm,
                          hipStream_t s) {
    const dim3 grd = cell_grid(p, 0);
    if (p.N == 3) k_stress_fields<3, false><<<grd, STRESS_BLOCK, 0, s>>>(p, m, u, strain, stress, vm);
    else if (aligned16(u)) k_stress_fields<2, true><<<grd, STRESS_BLOCK, 0, s>>>(p, m, u, strain, stress, vm);
    else k_stress_fields<2, false><<<grd, STRESS_BLOCK, 0, s>>>(p, m, u, strain, stress, vm);
    VFEM_HIP(hipGetLastError());
}

void launch_stress_pnorm(long long n, const double *vm, double P, double *partial, double *out, hipStream_t s) {
    k_stress_max_partial<<<STRESS_REDUCE_BLOCKS, 256, 0, s>>>(n, vm, partial);
    k_stress_max_finish<<<1, 256, 0, s>>>(STRESS_REDUCE_BLOCKS, partial, out);
    k_stress_power_partial<<<STRESS_REDUCE_BLOCKS, 256, 0, s>>>(n, vm, P, out, partial);
    k_stress_pnorm_finish<<<1, 256, 0, s>>>(STRESS_REDUCE_BLOCKS, partial, P, out);
    VFEM_HIP(hipGetLastError());
}

void launch_stress_adjoint_load(const StressProblem &p, const double *m, const double *u, double J, double P, const uint8_t *mask,
                                double *work, double *a, hipStream_t s) {
    const dim3 elems = cell_grid(p, 0), nodes = cell_grid(p, 1);
    const double invJ = 1.0 / J, pm1 = P - 1.0;
    const int ip = whole_exponent(pm1);
    if (p.N == 3) {
        k_stress_adjoint_elements<3, false><<<elems, STRESS_BLOCK, 0, s>>>(p, m, u, invJ, pm1, ip, work);
        k_stress_adjoint_gather<3><<<nodes, STRESS_BLOCK, 0, s>>>(p, work, mask, a);
    } else {
        if (aligned16(u)) k_stress_adjoint_elements<2, true><<<elems, STRESS_BLOCK, 0, s>>>(p, m, u, invJ, pm1, ip, work);
        else k_stress_adjoint_elements<2, false><<<elems, STRESS_BLOCK, 0, s>>>(p, m, u, invJ, pm1, ip, work);
        k_stress_adjoint_gather<2><<<nodes, STRESS_BLOCK, 0, s>>>(p, work, mask, a);
    }
    VFEM_HIP(hipGetLastError());
}

void launch_stress_gradient(const StressProblem &p, const double *K0, const double *m, const double *dm, const double *dE,
                            const double *u, const double *lambda, double J, double P, double *g, hipStream_t s) {
    const dim3 grd = cell_grid(p, 0);
    const double invJ = 1.0 / J, pm1 = P - 1.0;
    const int ip = whole_exponent(pm1);
    if (p.N == 3) k_stress_gradient<3, false><<<grd, STRESS_BLOCK, 0, s>>>(p, K0, m, dm, dE, u, lambda, invJ, pm1, ip, g);
    else if (aligned16(u) && aligned16(lambda)) k_stress_gradient<2, true><<<grd, STRESS_BLOCK, 0, s>>>(p, K0, m, dm, dE, u, lambda, invJ, pm1, ip, g);
    else k_stress_gradient<2, false><<<grd, STRESS_BLOCK, 0, s>>>(p, K0, m, dm, dE, u, lambda, invJ, pm1, ip, g);
    VFEM_HIP(hipGetLastError());
}

}  // namespace vfem
