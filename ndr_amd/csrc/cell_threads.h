// One thread per cell of a degree-1 grid (kernels_stress.hip, kernels_modal.hip, kernels_buckling.hip, kernels_loads.hip, and through
// thermal_device.h kernels_thermal.hip and kernels_thermal_mg.hip): a block is 64 lanes along the last (fastest) axis by 4 rows of
// the axis before it; in 3-D blockIdx.z walks axis 0.  A "cell" is an element (extra = 0) or a node (extra = 1) of a grid with
// ext[d] elements per axis.  Nodes and elements are numbered with the last axis fastest; element e owns the 2^N nodes (e_d + mu_d),
// its local node index has axis 0 as the most significant bit.
#pragma once
#include "vfem_internal.h"

namespace vfem {

// position (0 / 1) along axis d of local node a: axis 0 is the most significant bit
template <int N>
__device__ __forceinline__ constexpr int node_bit(int a, int d) { return (a >> (N - 1 - d)) & 1; }

// The 3^N nodes a node is coupled to (the node kernels of kernels_modal.hip and kernels_buckling.hip) are numbered in base 3.
// offset (-1 / 0 / 1) along axis d of neighbour k: axis 0 is the most significant base-3 digit
template <int N>
__device__ __forceinline__ constexpr int neighbour_offset(int k, int d) {
    int v = k;
    for (int i = N - 1; i > d; --i) v /= 3;
    return v % 3 - 1;
}

// the neighbour that local node j of the element in which this node is local node el stands for
template <int N>
__device__ __forceinline__ constexpr int neighbour_of(int el, int j) {
    int k = 0;
    for (int d = 0; d < N; ++d) k = 3 * k + (node_bit<N>(j, d) - node_bit<N>(el, d) + 1);
    return k;
}

// the thread's cell of a grid with `ext[d] + extra` cells per axis; false: outside
template <int N>
__device__ __forceinline__ bool thread_cell(const int *ext, int extra, int (&c)[N]) {
    c[N - 1] = blockIdx.x * 64 + threadIdx.x;
    c[N - 2] = blockIdx.y * 4 + threadIdx.y;
    if constexpr (N == 3) c[0] = blockIdx.z;
    bool in = true;
#pragma unroll
    for (int d = 0; d < N; ++d) in = in && c[d] < ext[d] + extra;
    return in;
}

template <int N>
__device__ __forceinline__ long long flat_index(const int *ext, int extra, const int (&c)[N]) {
    long long f = c[0];
#pragma unroll
    for (int d = 1; d < N; ++d) f = f * (ext[d] + extra) + c[d];
    return f;
}

// the launch that gives every cell its thread
inline dim3 cell_block() { return dim3(64, 4, 1); }
inline dim3 cell_grid(int N, const int *ne, int extra) {
    const dim3 grd((unsigned) (ne[N - 1] + extra + 63) / 64, (unsigned) (ne[N - 2] + extra + 3) / 4, N == 3 ? (unsigned) (ne[0] + extra) : 1u);
    if (grd.y > 65535u || grd.z > 65535u) throw Error("grid kernels: grid too large along an outer axis");
    return grd;
}

}  // namespace vfem
