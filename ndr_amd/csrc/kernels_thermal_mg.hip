// Kernels of the multigrid preconditioner of the scalar conduction operator (thermal_mg.h): the level masks, the
// Galerkin product of a level's couplings, the inverted diagonal, apply / residual / colour sweep over a level's couplings (stored,
// or level 0's matrix-free ones), the transfers and the dense matrix of the coarsest level.
//
// All fp64, one double per access (8-byte alignment is enough), no atomics: one thread owns what it writes and sums in a fixed order,
// so two runs give the same bits.  A level's couplings come from a source: ThermalFineSrc forms them from the node's 2^N
// conductivities as k_thermal_apply does (thermal_couplings, thermal_device.h), with the capacity term of a transient step's
// operator in instantiations of their own, ThermalStoredSrc loads A[offset][node] (coalesced over the nodes of a
// wave).  Both give the 3^N coefficients, the neighbour distances and the bits of the neighbours that take part.
//
// Level-0 colour sweep (the hot path: two sweeps of 2^N colours per cycle over all fine nodes): one thread per node of the colour,
// 64 x 4 blocks over the colour's sub-grid with the lanes along the last axis.  The lanes of a wave touch every second double of a
// row, and their -1 / +1 neighbours are the doubles in between, so every line of x the wave touches is used whole; b, 1 / diag and the
// store are strided by two (half of each line; the other colour of the row uses the other half from L2).  The stored levels take
// flat 256-thread blocks over the colour's nodes: their rows are short.
#include "thermal_mg.h"

#include "thermal_device.h"

#include <algorithm>

namespace vfem {

namespace {

constexpr int MG_T = 256;

// level 0: Extra is NoCapacity, or the CapacityTerm of a transient step's hierarchy (thermal_device.h).  The empty member takes no
// room and the full one sits behind K: the layouts the two forms had as separate types, and with them their code
template <class Extra>
struct ThermalFineSrc {
    ThermalMatrix K;
    [[no_unique_address]] Extra extra;
    const double *kappa;
    template <int N>
    __device__ __forceinline__ void couplings(const ModalGrid &g, const int (&c)[N], long long node,
                                              double (&coef)[ThermalTraits<N>::NB]) const {
        thermal_couplings<N>(g, K, kappa, extra, c, coef);
    }
};

struct ThermalStoredSrc {
    const double *A;
    template <int N>
    __device__ __forceinline__ void couplings(const ModalGrid &g, const int (&c)[N], long long node,
                                              double (&coef)[ThermalTraits<N>::NB]) const {
#pragma unroll
        for (int k = 0; k < ThermalTraits<N>::NB; ++k) coef[k] = A[k * g.nnode + node];
    }
};

// the thread's node of a colour (GsColor: first node, stride and count per axis); false: outside.  CELL: the 64 x 4 blocks of
// cell_threads.h over the colour's sub-grid; otherwise flat blocks of MG_T threads, last axis fastest
template <int N, bool CELL>
__device__ __forceinline__ bool colour_node(const GsColor &col, int (&c)[N]) {
    int t[N];
    if constexpr (CELL) {
        t[N - 1] = blockIdx.x * 64 + threadIdx.x;
        t[N - 2] = blockIdx.y * 4 + threadIdx.y;
        if constexpr (N == 3) t[0] = blockIdx.z;
    } else {
        long long f = (long long) blockIdx.x * MG_T + threadIdx.x;
#pragma unroll
        for (int d = N - 1; d > 0; --d) {
            t[d] = (int) (f % col.cnt[d]);
            f /= col.cnt[d];
        }
        t[0] = f < col.cnt[0] ? (int) f : col.cnt[0];
    }
    bool in = true;
#pragma unroll
    for (int d = 0; d < N; ++d) {
        in = in && t[d] < col.cnt[d];
        c[d] = col.start[d] + col.inc[d] * t[d];
    }
    return in;
}

GsColor all_nodes(const ModalGrid &g) {
    GsColor col{{0, 0, 0}, {1, 1, 1}, {1, 1, 1}};
    for (int d = 0; d < g.N; ++d) col.cnt[d] = g.ne[d] + 1;
    return col;
}

unsigned flat_blocks(const GsColor &col, int extra_factor = 1) {
    long long n = extra_factor;
    for (int d = 0; d < 3; ++d) n *= col.cnt[d];
    return (unsigned) ((n + MG_T - 1) / MG_T);
}

dim3 cell_blocks(int N, const GsColor &col) {
    const dim3 grd((unsigned) (col.cnt[N - 1] + 63) / 64, (unsigned) (col.cnt[N - 2] + 3) / 4, N == 3 ? (unsigned) col.cnt[0] : 1u);
    if (grd.y > 65535u || grd.z > 65535u) throw Error("thermal multigrid kernels: grid too large along an outer axis");
    return grd;
}

enum { MG_APPLY = 0, MG_RESIDUAL = 1, MG_SWEEP = 2 };

// MG_APPLY: out = A_l x.  MG_RESIDUAL: out = b - A_l x.  MG_SWEEP: x += dinv (b - A_l x) on the nodes of the colour (out is x, and is
// read: no __restrict__).  A fixed node's row is the identity, a fixed neighbour takes no part.
template <int N, int MODE, class Src, bool CELL>
__global__ void __launch_bounds__(256) k_thermal_mg_level(ModalGrid g, Src src, const uint8_t *__restrict__ fixed,
                                                          const double *__restrict__ dinv, GsColor col, const double *x,
                                                          const double *__restrict__ b, double *out) {
    constexpr int NB = ThermalTraits<N>::NB, SELF = ThermalTraits<N>::SELF;
    int c[N];
    if (!colour_node<N, CELL>(col, c)) return;
    const long long node = flat_index<N>(g.ne, 1, c);
    double coef[NB];
    src.template couplings<N>(g, c, node, coef);
    long long delta[NB];
    const unsigned live = thermal_live_neighbours<N>(g, fixed, c, node, delta);
    const double own = x[node];
    double acc = 0.0;
    if (!((live >> SELF) & 1u)) acc = own;
    else {
#pragma unroll
        for (int k = 0; k < NB; ++k)
            if ((live >> k) & 1u) acc = fma(coef[k], x[node + delta[k]], acc);
    }
    if constexpr (MODE == MG_APPLY) out[node] = acc;
    else if constexpr (MODE == MG_RESIDUAL) out[node] = b[node] - acc;
    else out[node] = fma(b[node] - acc, dinv[node], own);
}

__global__ void __launch_bounds__(MG_T) k_thermal_mg_normalise_mask(long long n, const uint8_t *__restrict__ in, uint8_t *__restrict__ out) {
    const long long i = (long long) blockIdx.x * MG_T + threadIdx.x;
    if (i < n) out[i] = in[i] ? 1 : 0;
}

template <int N>
__global__ void __launch_bounds__(MG_T) k_thermal_mg_coarsen_mask(ModalGrid gf, ModalGrid gc, GsColor all, const uint8_t *__restrict__ ff,
                                                                  uint8_t *__restrict__ fc) {
    int c[N], f[N];
    if (!colour_node<N, false>(all, c)) return;
#pragma unroll
    for (int d = 0; d < N; ++d) f[d] = 2 * c[d];
    fc[flat_index<N>(gc.ne, 1, c)] = ff[flat_index<N>(gf.ne, 1, f)];
}

// one thread per coarse offset O and coarse node I.  Per axis the fine row node is a = 2 I + da (weight 1 or 1/2), the fine column
// node b = a + of, and b lies in the support of coarse node I + O when db = da + of - 2 O is -1, 0 or +1 (weight 1 or 1/2).  Fine rows
// in ascending da, columns in ascending offset within: a fixed order.  The loop over the rows stays rolled (each forms 3^N
// couplings); the loop over a row's offsets is unrolled so that the couplings stay in registers.
template <int N, class Src>
__global__ void __launch_bounds__(MG_T) k_thermal_mg_galerkin(ModalGrid gf, ModalGrid gc, Src src, GsColor all,
                                                              const uint8_t *__restrict__ ff, const uint8_t *__restrict__ fc,
                                                              double *__restrict__ Ac) {
    constexpr int NB = ThermalTraits<N>::NB;
    // blockIdx.y is the coarse offset
    const int O = blockIdx.y;
    int Ic[N], Od[N];
    if (!colour_node<N, false>(all, Ic)) return;
    const long long I = flat_index<N>(gc.ne, 1, Ic);
    bool coarse_free = !fc[I];
    long long J = 0;
#pragma unroll
    for (int d = 0; d < N; ++d) {
        Od[d] = neighbour_offset<N>(O, d);
        const int j = Ic[d] + Od[d];
        coarse_free = coarse_free && j >= 0 && j <= gc.ne[d];
        J = J * (gc.ne[d] + 1) + j;
    }
    if (coarse_free) coarse_free = !fc[J];
    double acc = 0.0;
    if (coarse_free) {
#pragma unroll 1
        for (int ia = 0; ia < NB; ++ia) {
            int da[N], a[N];
            double wa = 1.0;
            bool in = true;
            {
                int v = ia;
#pragma unroll
                for (int d = N - 1; d >= 0; --d, v /= 3) {
                    da[d] = v % 3 - 1;
                    if (da[d] != 0) wa *= 0.5;
                    a[d] = 2 * Ic[d] + da[d];
                    in = in && a[d] >= 0 && a[d] <= gf.ne[d];
                }
            }
            if (!in) continue;
            const long long node = flat_index<N>(gf.ne, 1, a);
            if (ff[node]) continue;
            double coef[NB];
            src.template couplings<N>(gf, a, node, coef);
            long long delta[NB];
            const unsigned live = thermal_live_neighbours<N>(gf, ff, a, node, delta);
#pragma unroll
            for (int io = 0; io < NB; ++io) {
                double wb = wa;
                bool reach = (live >> io) & 1u;
#pragma unroll
                for (int d = 0; d < N; ++d) {
                    const int db = da[d] + neighbour_offset<N>(io, d) - 2 * Od[d];
                    if (db < -1 || db > 1) reach = false;
                    if (db != 0) wb *= 0.5;
                }
                if (reach) acc = fma(wb, coef[io], acc);
            }
        }
    }
    Ac[O * gc.nnode + I] = acc;
}

template <int N>
__global__ void __launch_bounds__(MG_T) k_thermal_mg_dinv(long long n, const double *__restrict__ A, const uint8_t *__restrict__ fixed,
                                                          double *__restrict__ dinv) {
    const long long i = (long long) blockIdx.x * MG_T + threadIdx.x;
    if (i >= n) return;
    dinv[i] = fixed[i] ? 1.0 : 1.0 / A[ThermalTraits<N>::SELF * n + i];
}

// fine nodes 2 J - 1, 2 J, 2 J + 1 per axis with weights 1/2, 1, 1/2, in ascending offset; fixed fine nodes take no part
template <int N>
__global__ void __launch_bounds__(MG_T) k_thermal_mg_restrict(ModalGrid gf, ModalGrid gc, GsColor all, const uint8_t *__restrict__ ff,
                                                              const uint8_t *__restrict__ fc, const double *__restrict__ vf,
                                                              double *__restrict__ vc) {
    int Jc[N];
    if (!colour_node<N, false>(all, Jc)) return;
    const long long J = flat_index<N>(gc.ne, 1, Jc);
    double acc = 0.0;
    if (!fc[J]) {
#pragma unroll
        for (int o = 0; o < ThermalTraits<N>::NB; ++o) {
            int a[N];
            double w = 1.0;
            bool in = true;
#pragma unroll
            for (int d = 0; d < N; ++d) {
                const int k = neighbour_offset<N>(o, d);
                a[d] = 2 * Jc[d] + k;
                if (k != 0) w *= 0.5;
                in = in && a[d] >= 0 && a[d] <= gf.ne[d];
            }
            if (!in) continue;
            const long long node = flat_index<N>(gf.ne, 1, a);
            if (!ff[node]) acc = fma(w, vf[node], acc);
        }
    }
    vc[J] = acc;
}

// an even fine index 2 j takes coarse j, an odd one 2 j + 1 coarse j and j + 1 with 1/2 each; fixed coarse nodes count as zero
template <int N>
__global__ void __launch_bounds__(MG_T) k_thermal_mg_prolong_add(ModalGrid gf, ModalGrid gc, GsColor all, const uint8_t *__restrict__ ff,
                                                                 const uint8_t *__restrict__ fc, const double *__restrict__ vc,
                                                                 double *__restrict__ vf) {
    int a[N];
    if (!colour_node<N, false>(all, a)) return;
    const long long node = flat_index<N>(gf.ne, 1, a);
    if (ff[node]) return;
    double acc = 0.0;
#pragma unroll
    for (int m = 0; m < (1 << N); ++m) {
        int j[N];
        double w = 1.0;
        bool used = true;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            const int bit = node_bit<N>(m, d), odd = a[d] & 1;
            if (bit && !odd) used = false;
            if (odd) w *= 0.5;
            j[d] = (a[d] >> 1) + bit;
        }
        if (!used) continue;                    // (an odd index is at most ne - 1: j + 1 is a coarse node)
        const long long J = flat_index<N>(gc.ne, 1, j);
        if (!fc[J]) acc = fma(w, vc[J], acc);
    }
    vf[node] += acc;
}

// one thread per node writes the node's row
template <int N, class Src>
__global__ void __launch_bounds__(MG_T) k_thermal_mg_dense(ModalGrid g, Src src, GsColor all, const uint8_t *__restrict__ fixed,
                                                           double *__restrict__ M) {
    constexpr int NB = ThermalTraits<N>::NB, SELF = ThermalTraits<N>::SELF;
    int c[N];
    if (!colour_node<N, false>(all, c)) return;
    const long long node = flat_index<N>(g.ne, 1, c);
    double coef[NB];
    src.template couplings<N>(g, c, node, coef);
    long long delta[NB];
    const unsigned live = thermal_live_neighbours<N>(g, fixed, c, node, delta);
    double *row = M + node * g.nnode + node;
    if (!((live >> SELF) & 1u)) { row[0] = 1.0; return; }
#pragma unroll
    for (int k = 0; k < NB; ++k)
        if ((live >> k) & 1u) row[delta[k]] = coef[k];
}

__global__ void __launch_bounds__(MG_T) k_thermal_mg_copy_fixed(long long n, const uint8_t *__restrict__ fixed, const double *__restrict__ b,
                                                                double *__restrict__ x) {
    const long long i = (long long) blockIdx.x * MG_T + threadIdx.x;
    if (i < n && fixed[i]) x[i] = b[i];
}

unsigned blocks_for(long long n) { return (unsigned) std::max<long long>(1, (n + MG_T - 1) / MG_T); }

}  // namespace

#define THERMAL_MG_DISPATCH(g, call2, call3) do { if ((g).N == 2) { call2; } else { call3; } VFEM_HIP(hipGetLastError()); } while (0)

// launch(src) with the source object of a level's operator: the stored stencil, or level 0 in its one-term or two-term form
template <class Launch>
void with_source(const ThermalLevelOp &op, const Launch &launch) {
    if (!op.fine) launch(ThermalStoredSrc{op.A});
    else if (op.fine->cap) launch(ThermalFineSrc<CapacityTerm>{op.fine->K, {op.fine->mb, op.fine->cap}, op.fine->kappa});
    else launch(ThermalFineSrc<NoCapacity>{op.fine->K, {}, op.fine->kappa});
}

void launch_thermal_mg_normalise_mask(long long n, const uint8_t *in, uint8_t *out, hipStream_t s) {
    k_thermal_mg_normalise_mask<<<blocks_for(n), MG_T, 0, s>>>(n, in, out);
    VFEM_HIP(hipGetLastError());
}

void launch_thermal_mg_coarsen_mask(const ModalGrid &fine, const ModalGrid &coarse, const uint8_t *fixed_f, uint8_t *fixed_c, hipStream_t s) {
    const GsColor all = all_nodes(coarse);
    THERMAL_MG_DISPATCH(fine, (k_thermal_mg_coarsen_mask<2><<<flat_blocks(all), MG_T, 0, s>>>(fine, coarse, all, fixed_f, fixed_c)),
                        (k_thermal_mg_coarsen_mask<3><<<flat_blocks(all), MG_T, 0, s>>>(fine, coarse, all, fixed_f, fixed_c)));
}

void launch_thermal_mg_galerkin(const ModalGrid &fine, const ModalGrid &coarse, const ThermalLevelOp &src, const uint8_t *fixed_f,
                                const uint8_t *fixed_c, double *Ac, hipStream_t s) {
    const GsColor all = all_nodes(coarse);
    const dim3 grd(flat_blocks(all), fine.N == 2 ? 9 : 27);
    with_source(src, [&](auto f) {
        using Src = decltype(f);
#define ARGS <<<grd, MG_T, 0, s>>>(fine, coarse, f, all, fixed_f, fixed_c, Ac)
        THERMAL_MG_DISPATCH(fine, (k_thermal_mg_galerkin<2, Src> ARGS), (k_thermal_mg_galerkin<3, Src> ARGS));
#undef ARGS
    });
}

void launch_thermal_mg_dinv(const ModalGrid &g, const double *A, const uint8_t *fixed, double *dinv, hipStream_t s) {
    THERMAL_MG_DISPATCH(g, (k_thermal_mg_dinv<2><<<blocks_for(g.nnode), MG_T, 0, s>>>(g.nnode, A, fixed, dinv)),
                        (k_thermal_mg_dinv<3><<<blocks_for(g.nnode), MG_T, 0, s>>>(g.nnode, A, fixed, dinv)));
}

void launch_thermal_mg_apply(const ModalGrid &g, const double *A, const uint8_t *fixed, const double *x, const double *b, double *out,
                             hipStream_t s) {
    const GsColor all = all_nodes(g);
    const ThermalStoredSrc f{A};
#define ARGS <<<flat_blocks(all), MG_T, 0, s>>>(g, f, fixed, nullptr, all, x, b, out)
    if (b) THERMAL_MG_DISPATCH(g, (k_thermal_mg_level<2, MG_RESIDUAL, ThermalStoredSrc, false> ARGS), (k_thermal_mg_level<3, MG_RESIDUAL, ThermalStoredSrc, false> ARGS));
    else THERMAL_MG_DISPATCH(g, (k_thermal_mg_level<2, MG_APPLY, ThermalStoredSrc, false> ARGS), (k_thermal_mg_level<3, MG_APPLY, ThermalStoredSrc, false> ARGS));
#undef ARGS
}

void launch_thermal_mg_sweep_colour(const ModalGrid &g, const ThermalLevelOp &src, const uint8_t *fixed, const double *dinv,
                                    const GsColor &colour, double *x, const double *b, hipStream_t s) {
    // level 0 takes the 64 x 4 blocks of the cell kernels, a stored level flat ones: its rows are short
    with_source(src, [&](auto f) {
        using Src = decltype(f);
        constexpr bool CELL = !std::is_same<Src, ThermalStoredSrc>::value;
        const dim3 grd = CELL ? cell_blocks(g.N, colour) : dim3(flat_blocks(colour)), blk = CELL ? cell_block() : dim3(MG_T);
#define ARGS <<<grd, blk, 0, s>>>(g, f, fixed, dinv, colour, x, b, x)
        THERMAL_MG_DISPATCH(g, (k_thermal_mg_level<2, MG_SWEEP, Src, CELL> ARGS), (k_thermal_mg_level<3, MG_SWEEP, Src, CELL> ARGS));
#undef ARGS
    });
}

void launch_thermal_mg_restrict(const ModalGrid &fine, const ModalGrid &coarse, const uint8_t *fixed_f, const uint8_t *fixed_c,
                                const double *vf, double *vc, hipStream_t s) {
    const GsColor all = all_nodes(coarse);
#define ARGS <<<flat_blocks(all), MG_T, 0, s>>>(fine, coarse, all, fixed_f, fixed_c, vf, vc)
    THERMAL_MG_DISPATCH(fine, (k_thermal_mg_restrict<2> ARGS), (k_thermal_mg_restrict<3> ARGS));
#undef ARGS
}

void launch_thermal_mg_prolong_add(const ModalGrid &fine, const ModalGrid &coarse, const uint8_t *fixed_f, const uint8_t *fixed_c,
                                   const double *vc, double *vf, hipStream_t s) {
    const GsColor all = all_nodes(fine);
#define ARGS <<<flat_blocks(all), MG_T, 0, s>>>(fine, coarse, all, fixed_f, fixed_c, vc, vf)
    THERMAL_MG_DISPATCH(fine, (k_thermal_mg_prolong_add<2> ARGS), (k_thermal_mg_prolong_add<3> ARGS));
#undef ARGS
}

void launch_thermal_mg_dense(const ModalGrid &g, const ThermalLevelOp &src, const uint8_t *fixed, double *M, hipStream_t s) {
    const GsColor all = all_nodes(g);
    with_source(src, [&](auto f) {
        using Src = decltype(f);
#define ARGS <<<flat_blocks(all), MG_T, 0, s>>>(g, f, all, fixed, M)
        THERMAL_MG_DISPATCH(g, (k_thermal_mg_dense<2, Src> ARGS), (k_thermal_mg_dense<3, Src> ARGS));
#undef ARGS
    });
}

void launch_thermal_mg_copy_fixed(long long n, const uint8_t *fixed, const double *b, double *x, hipStream_t s) {
    k_thermal_mg_copy_fixed<<<blocks_for(n), MG_T, 0, s>>>(n, fixed, b, x);
    VFEM_HIP(hipGetLastError());
}

}  // namespace vfem
