// Device code that kernels_thermal.hip, kernels_thermal_mg.hip and kernels_transient.hip share: how a node of the
// matrix-free scalar operator forms its couplings and finds the neighbours that take part.  Said once, so that the apply, the
// level-0 colour sweep, the Galerkin product from level 0 and the dense fill of a one-level hierarchy sum the same terms in the same
// order, for the conduction operator and for the two-term operator of a transient step alike.
//
// The two bodies are macros that the functions below wrap.  k_thermal_apply<3> sits at the edge of its register budget (63 VGPRs,
// 106 SGPRs, no scratch): with the arrays handed to a function by reference the compiler schedules it differently, even though
// everything is inlined (measured: 64 VGPRs and 68 bytes of scratch per lane with the couplings in a function, 196 bytes with the
// neighbours in one too).  Expanded in the kernel's own body the macros give the code the kernel had before the move, register for
// register.
#pragma once
#include "thermal.h"

#include "cell_threads.h"

namespace vfem {

template <int N>
struct ThermalTraits {
    static constexpr int NPE = 1 << N;
    static constexpr int NB = N == 2 ? 9 : 27;          // nodes coupled to a node
    static constexpr int SELF = (NB - 1) / 2;
};

// kappa of the element in which the node at c is local node el; 0 outside the grid
template <int N>
__device__ __forceinline__ double incident_kappa(const ModalGrid &g, const double *__restrict__ kappa, const int (&c)[N], int el) {
    int ec[N];
    bool in = true;
#pragma unroll
    for (int d = 0; d < N; ++d) {
        ec[d] = c[d] - node_bit<N>(el, d);
        in = in && ec[d] >= 0 && ec[d] < g.ne[d];
    }
    return in ? kappa[flat_index<N>(g.ne, 0, ec)] : 0.0;
}

// coef[k] (double [3^N]) = the coupling of the node at c with its neighbour k (cell_threads.h: neighbour_offset) in
// sum_e kappa[e] Kc0, before any mask: the sum over the elements that hold both of kappa[e] Kc0[el][j], elements in ascending local
// index el, j ascending within
#define VFEM_THERMAL_COUPLINGS(N, g, K, kappa, c, coef)                                                                                \
    do {                                                                                                                               \
        _Pragma("unroll") for (int k_ = 0; k_ < ThermalTraits<N>::NB; ++k_) coef[k_] = 0.0;                                            \
        _Pragma("unroll") for (int el_ = 0; el_ < ThermalTraits<N>::NPE; ++el_) {                                                      \
            const double ke_ = incident_kappa<N>(g, kappa, c, el_);                                                                    \
            _Pragma("unroll") for (int j_ = 0; j_ < ThermalTraits<N>::NPE; ++j_)                                                       \
                coef[neighbour_of<N>(el_, j_)] = fma(ke_, K.k[el_ * ThermalTraits<N>::NPE + j_], coef[neighbour_of<N>(el_, j_)]);      \
        }                                                                                                                              \
    } while (0)

// The two-term form of the transient operator (transient.h): the coupling in sum_e (kappa[e] Ka + cap[e] M(mb)), where
// M(mb)[el][j] = mb.m[popcount(el xor j)] depends only on the number of axes along which the two local nodes differ.  The same loop
// order as above; each pair adds its conduction term first and its capacity term second
#define VFEM_TRANSIENT_COUPLINGS(N, g, K, mb, kappa, cap, c, coef)                                                                     \
    do {                                                                                                                               \
        _Pragma("unroll") for (int k_ = 0; k_ < ThermalTraits<N>::NB; ++k_) coef[k_] = 0.0;                                            \
        _Pragma("unroll") for (int el_ = 0; el_ < ThermalTraits<N>::NPE; ++el_) {                                                      \
            const double ke_ = incident_kappa<N>(g, kappa, c, el_);                                                                    \
            const double ce_ = incident_kappa<N>(g, cap, c, el_);                                                                      \
            _Pragma("unroll") for (int j_ = 0; j_ < ThermalTraits<N>::NPE; ++j_) {                                                     \
                coef[neighbour_of<N>(el_, j_)] = fma(ke_, K.k[el_ * ThermalTraits<N>::NPE + j_], coef[neighbour_of<N>(el_, j_)]);      \
                coef[neighbour_of<N>(el_, j_)] = fma(ce_, mb.m[__builtin_popcount(el_ ^ j_)], coef[neighbour_of<N>(el_, j_)]);         \
            }                                                                                                                          \
        }                                                                                                                              \
    } while (0)

// delta[k] (long long [3^N]) = the node index of neighbour k minus this node's; live (unsigned, 0 on entry) gets the bits of the
// neighbours that lie inside the grid and are not fixed (bit SELF: the node itself is free); fixed may be null
#define VFEM_THERMAL_LIVE_NEIGHBOURS(N, g, fixed, c, node, delta, live)                                                                \
    do {                                                                                                                               \
        _Pragma("unroll") for (int k_ = 0; k_ < ThermalTraits<N>::NB; ++k_) {                                                          \
            bool in_ = true;                                                                                                           \
            long long off_ = 0;                                                                                                        \
            _Pragma("unroll") for (int d_ = 0; d_ < N; ++d_) {                                                                         \
                const int o_ = neighbour_offset<N>(k_, d_);                                                                            \
                in_ = in_ && c[d_] + o_ >= 0 && c[d_] + o_ <= g.ne[d_];                                                                \
                off_ = off_ * (g.ne[d_] + 1) + o_;                                                                                     \
            }                                                                                                                          \
            delta[k_] = off_;                                                                                                          \
            if (in_ && !(fixed && fixed[node + off_])) live |= 1u << k_;                                                               \
        }                                                                                                                              \
    } while (0)

template <int N>
__device__ __forceinline__ void thermal_couplings(const ModalGrid &g, const ThermalMatrix &K, const double *__restrict__ kappa,
                                                  const int (&c)[N], double (&coef)[ThermalTraits<N>::NB]) {
    VFEM_THERMAL_COUPLINGS(N, g, K, kappa, c, coef);
}

template <int N>
__device__ __forceinline__ void transient_couplings(const ModalGrid &g, const ThermalMatrix &K, const ThermalCapacity &mb,
                                                    const double *__restrict__ kappa, const double *__restrict__ cap, const int (&c)[N],
                                                    double (&coef)[ThermalTraits<N>::NB]) {
    VFEM_TRANSIENT_COUPLINGS(N, g, K, mb, kappa, cap, c, coef);
}

template <int N>
__device__ __forceinline__ unsigned thermal_live_neighbours(const ModalGrid &g, const uint8_t *__restrict__ fixed, const int (&c)[N],
                                                            long long node, long long (&delta)[ThermalTraits<N>::NB]) {
    unsigned live = 0u;
    VFEM_THERMAL_LIVE_NEIGHBOURS(N, g, fixed, c, node, delta, live);
    return live;
}

}  // namespace vfem
