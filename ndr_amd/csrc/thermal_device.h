// Device code that kernels_thermal.hip and kernels_thermal_mg.hip share: how a node of the matrix-free scalar
// operator forms its couplings and finds the neighbours that take part.  Said once, so that the apply, the level-0 colour sweep, the
// Galerkin product from level 0 and the dense fill of a one-level hierarchy sum the same terms in the same order.  The one-term and
// the two-term form of the operator (thermal.h) are two instantiations of the same text: `if constexpr` leaves the capacity lines out
// of the one-term code, and what only the two-term form takes (mb, cap) has the empty type NoCapacity in the one-term instantiation.
//
// The two bodies are macros that the functions below wrap.  k_thermal_apply<3> sits at the edge of its register budget (one-term:
// 63 VGPRs, no scratch): with the arrays handed to a function by reference the compiler schedules it differently, even though
// everything is inlined (measured: 64 VGPRs and 68 bytes of scratch per lane with the couplings in a function, 196 bytes with the
// neighbours in one too; a shared inlined body behind two thin kernels, or the operator as one struct argument, cost registers or
// lane spills in the same way: DESIGN 3.18).  Expanded in the kernel's own body the macros give the code the kernel had before the
// move, register for register.
#pragma once
#include "thermal.h"

#include "cell_threads.h"

#include <type_traits>

namespace vfem {

template <int N>
struct ThermalTraits {
    static constexpr int NPE = 1 << N;
    static constexpr int NB = N == 2 ? 9 : 27;          // nodes coupled to a node
    static constexpr int SELF = (NB - 1) / 2;
};

// The type of a kernel argument that only the two-term form has: T there, and an empty placeholder in the one-term instantiation
// (never read: every use is behind `if constexpr (TWO)`).  The arguments stay flat and in one order for both forms: handing the
// operator over as one struct costs k_thermal_apply<3> lane spills.
struct NoCapacity {};
template <bool TWO, class T>
using OnlyTwoTerm = std::conditional_t<TWO, T, NoCapacity>;
// the capacity term as a member of a multigrid source (kernels_thermal_mg.hip), where Extra is this or NoCapacity
struct CapacityTerm {
    ThermalCapacity mb;
    const double *cap;
};
template <class Extra>
constexpr bool has_capacity = !std::is_same<Extra, NoCapacity>::value;

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
// sum_e (kappa[e] K + cap[e] M(mb)), before any mask: the sum over the elements that hold both of kappa[e] K[el][j], and with TWO of
// cap[e] mb.m[popcount(el xor j)], elements in ascending local index el, j ascending within; each pair adds its conduction term
// first and its capacity term second.  (mb and cap are read only under TWO.)
#define VFEM_THERMAL_COUPLINGS(N, TWO, g, K, mb, kappa, cap, c, coef)                                                                  \
    do {                                                                                                                               \
        _Pragma("unroll") for (int k_ = 0; k_ < ThermalTraits<N>::NB; ++k_) coef[k_] = 0.0;                                            \
        _Pragma("unroll") for (int el_ = 0; el_ < ThermalTraits<N>::NPE; ++el_) {                                                      \
            const double ke_ = incident_kappa<N>(g, kappa, c, el_);                                                                    \
            [[maybe_unused]] double ce_ = 0.0;                                                                                         \
            if constexpr (TWO) ce_ = incident_kappa<N>(g, cap, c, el_);                                                                \
            _Pragma("unroll") for (int j_ = 0; j_ < ThermalTraits<N>::NPE; ++j_) {                                                     \
                coef[neighbour_of<N>(el_, j_)] = fma(ke_, K.k[el_ * ThermalTraits<N>::NPE + j_], coef[neighbour_of<N>(el_, j_)]);      \
                if constexpr (TWO)                                                                                                     \
                    coef[neighbour_of<N>(el_, j_)] = fma(ce_, mb.m[__builtin_popcount(el_ ^ j_)], coef[neighbour_of<N>(el_, j_)]);     \
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

template <int N, class Extra>
__device__ __forceinline__ void thermal_couplings(const ModalGrid &g, const ThermalMatrix &K, const double *__restrict__ kappa,
                                                  const Extra &extra, const int (&c)[N], double (&coef)[ThermalTraits<N>::NB]) {
    VFEM_THERMAL_COUPLINGS(N, has_capacity<Extra>, g, K, extra.mb, kappa, extra.cap, c, coef);
}

template <int N>
__device__ __forceinline__ unsigned thermal_live_neighbours(const ModalGrid &g, const uint8_t *__restrict__ fixed, const int (&c)[N],
                                                            long long node, long long (&delta)[ThermalTraits<N>::NB]) {
    unsigned live = 0u;
    VFEM_THERMAL_LIVE_NEIGHBOURS(N, g, fixed, c, node, delta, live);
    return live;
}

}  // namespace vfem
