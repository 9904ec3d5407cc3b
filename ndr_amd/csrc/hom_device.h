// Device helpers of the periodic-homogenisation kernels (kernels_hom.hip, kernels_hom_mg.hip): the periodic node grid, the moduli of
// a node's incident elements, the N x N coefficient block of a neighbour offset, the inverse of a node block and the two-stage
// reductions.  Each is written once, here.
#pragma once
#include "hom.h"

#include "device_utils.h"

namespace vfem {

namespace {

constexpr int HOM_T = HOM_THREADS;

template <int N>
struct HomDims {
    int n[N];
    int pn;
};

template <int N>
struct HomTraits {
    static constexpr int S = N == 2 ? 3 : 6;
    static constexpr int NPE = 1 << N;
    static constexpr int KE = N * NPE;
    static constexpr int NOFF = N == 2 ? 9 : 27;
};

// position (0 / 1) along axis d of local node a: axis 0 is the most significant bit (the last axis runs fastest)
template <int N>
__host__ __device__ constexpr int axis_bit(int a, int d) { return (a >> (N - 1 - d)) & 1; }

template <int N>
__device__ __forceinline__ int hom_flat(const HomDims<N> &g, const int c[N]) {
    int f = c[0];
#pragma unroll
    for (int d = 1; d < N; ++d) f = f * g.n[d] + c[d];
    return f;
}

// coordinates of periodic node / element t and, per axis, the wrapped coordinates at offsets -1, 0, +1
template <int N>
__device__ __forceinline__ void hom_neighbours(int t, const HomDims<N> &g, int nb[N][3]) {
#pragma unroll
    for (int d = N - 1; d >= 0; --d) {
        const int c = t % g.n[d];
        t /= g.n[d];
        nb[d][0] = c == 0 ? g.n[d] - 1 : c - 1;
        nb[d][1] = c;
        nb[d][2] = c + 1 == g.n[d] ? 0 : c + 1;
    }
}

// moduli of the 2^N elements incident to a node: in element a the node is local node a, i.e. the element sits one step
// back along every axis whose bit is set
template <int N>
__device__ __forceinline__ void hom_incident_moduli(const HomDims<N> &g, const int nb[N][3], const double *__restrict__ E,
                                                    double Ee[1 << N]) {
#pragma unroll
    for (int a = 0; a < (1 << N); ++a) {
        int c[N];
#pragma unroll
        for (int d = 0; d < N; ++d) c[d] = nb[d][1 - axis_bit<N>(a, d)];
        Ee[a] = E[hom_flat<N>(g, c)];
    }
}

// flat indices of the 2^N nodes of element t (its first node has the element's own coordinates)
template <int N>
__device__ __forceinline__ void hom_element_nodes(const HomDims<N> &g, const int nb[N][3], int nd[1 << N]) {
#pragma unroll
    for (int m = 0; m < (1 << N); ++m) {
        int c[N];
#pragma unroll
        for (int d = 0; d < N; ++d) c[d] = nb[d][1 + axis_bit<N>(m, d)];
        nd[m] = hom_flat<N>(g, c);
    }
}

// sum of M per-thread values over the block, in a fixed order; thread m < M writes value m to partial[m * stride + block]
template <int M>
__device__ __forceinline__ void block_reduce_store(double (&v)[M], double *__restrict__ partial, int stride) {
    static_assert(M <= HOM_T, "one thread per value in the last step");
    __shared__ double sh[M][HOM_T / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        double x = v[m];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if (lane == 0) sh[m][wave] = x;
    }
    __syncthreads();
    if ((int) threadIdx.x < M) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < HOM_T / 64; ++w) s += sh[threadIdx.x][w];
        partial[(long long) threadIdx.x * stride + blockIdx.x] = s;
    }
}

// sum of nb partials by one block of HOM_T threads, in a fixed order; every thread returns the sum
__device__ __forceinline__ double sum_partials(const double *__restrict__ src, int nb) {
    __shared__ double sh[HOM_T];
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += HOM_T) s += src[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = HOM_T / 2; w > 0; w >>= 1) {
        if ((int) threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// B = scale sum_e E_e tab[e]: the N x N coefficient block of one neighbour offset from that offset's 2^N x N x N slice of the stencil
// table (scale: 0 for the pin's column, else 1)
template <int N>
__device__ __forceinline__ void hom_offset_block(const double (&Ee)[1 << N], const double *tab, double scale, double (&B)[N][N]) {
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) {
            double v = 0.0;
#pragma unroll
            for (int ln = 0; ln < (1 << N); ++ln) v += Ee[ln] * tab[(ln * N + a) * N + b];
            B[a][b] = v * scale;
        }
}

// I = B^-1 by cofactors
template <int N>
__device__ __forceinline__ void hom_invert_block(const double (&B)[N][N], double (&I)[N][N]) {
    if constexpr (N == 2) {
        const double r = 1.0 / (B[0][0] * B[1][1] - B[0][1] * B[1][0]);
        I[0][0] = B[1][1] * r; I[0][1] = -B[0][1] * r;
        I[1][0] = -B[1][0] * r; I[1][1] = B[0][0] * r;
    } else {
        const double c00 = B[1][1] * B[2][2] - B[1][2] * B[2][1], c01 = B[1][2] * B[2][0] - B[1][0] * B[2][2],
                     c02 = B[1][0] * B[2][1] - B[1][1] * B[2][0];
        const double r = 1.0 / (B[0][0] * c00 + B[0][1] * c01 + B[0][2] * c02);
        I[0][0] = c00 * r; I[1][0] = c01 * r; I[2][0] = c02 * r;
        I[0][1] = (B[0][2] * B[2][1] - B[0][1] * B[2][2]) * r;
        I[1][1] = (B[0][0] * B[2][2] - B[0][2] * B[2][0]) * r;
        I[2][1] = (B[0][1] * B[2][0] - B[0][0] * B[2][1]) * r;
        I[0][2] = (B[0][1] * B[1][2] - B[0][2] * B[1][1]) * r;
        I[1][2] = (B[0][2] * B[1][0] - B[0][0] * B[1][2]) * r;
        I[2][2] = (B[0][0] * B[1][1] - B[0][1] * B[1][0]) * r;
    }
}

template <int N>
HomDims<N> dims_of(const HomProblem &p) {
    HomDims<N> g;
    for (int d = 0; d < N; ++d) g.n[d] = p.n[d];
    g.pn = p.pn;
    return g;
}

}  // namespace

}  // namespace vfem
