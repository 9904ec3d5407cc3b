// Heat conduction on a degree-1 grid (thermal.h): the scalar operator
// A = P (sum_e kappa_e K + sum_e cap_e M(mb)) P + iota (I - P) on a block of nodal fields, its diagonal and its band for the direct
// solver, each kernel instantiated for the one-term form of the steady problem (no capacity term, iota = 1) and for the two-term form
// of a transient step; the load of a volumetric source, the density gradient of a sum of bilinear forms and the centre flux.
//
// All of them stream fp64 and do little arithmetic per byte.  Every sum has a fixed order and no kernel uses an atomic: the same
// bits run to run.  Device pointers need 8-byte alignment only (every access is one double).  K (at most 64 doubles) and mb (4
// doubles) travel in the kernel arguments: unrolled code reads them by uniform loads, the band kernel indexes them per lane.
//
// Apply: one thread per NODE (cell_threads.h), all columns: k_modal_mass_apply's form.  The coupling of the pair (node, node + o) is
// the sum over the elements that hold both of kappa[e] Kc0[el][j], el the node's local index there and j the neighbour's.  The
// thread forms these 3^N coefficients once from its 2^N conductivities (elements in ascending el, j ascending within) and then
// walks the columns: 3^N loads of X and one store per column.  A fixed node gives iota times its own value; a fixed neighbour is
// skipped.  The two-term form adds cap[e] M[el][j] to every coupling, the conduction term first.
// (A branch-free column loop -- coefficient 0 and offset 0 for a neighbour that takes no part, all 3^N loads issued together -- was
// tried and measured: 132 VGPRs and 3 waves per SIMD in 3-D, one column 0.71 ms against 0.47 ms on 256 x 256 x 128, eight columns 1.91
// against 2.23 ms.  The solver applies one column, so the predicated form stays)
//
// Gradient and flux: one thread per ELEMENT; the 2^N nodal values of a column are loaded once.
#include "thermal_device.h"

#include <algorithm>

namespace vfem {

namespace {

// (the node's couplings and the neighbours that take part: thermal_device.h, shared with the multigrid kernels; expanded here as
// macros, and the body of both forms here and not in a shared function, which keeps this kernel's registers where they were.
// TWO: the two-term form; the one-term form has iota = 1 and b for a residual as compile-time facts)
template <int N, bool TWO>
__global__ void __launch_bounds__(256) k_thermal_apply(ModalGrid g, ThermalMatrix K, OnlyTwoTerm<TWO, ThermalCapacity> mb,
                                                       const double *__restrict__ kappa,
                                                       OnlyTwoTerm<TWO, const double *__restrict__> cap,
                                                       const uint8_t *__restrict__ fixed, OnlyTwoTerm<TWO, int> identity, int ncols,
                                                       const double *__restrict__ X, const double *__restrict__ b,
                                                       OnlyTwoTerm<TWO, int> residual, double *__restrict__ Y) {
    constexpr int NB = ThermalTraits<N>::NB, SELF = ThermalTraits<N>::SELF;
    int c[N];
    if (!thread_cell<N>(g.ne, 1, c)) return;
    const long long node = flat_index<N>(g.ne, 1, c);
    double coef[NB];
    VFEM_THERMAL_COUPLINGS(N, TWO, g, K, mb, kappa, cap, c, coef);
    long long delta[NB];            // the neighbour's node index minus this one's
    unsigned live = 0u;             // neighbours inside the grid that are not fixed
    VFEM_THERMAL_LIVE_NEIGHBOURS(N, g, fixed, c, node, delta, live);
    const bool self_fixed = !((live >> SELF) & 1u);
    for (int col = 0; col < ncols; ++col) {
        const double *__restrict__ x = X + col * g.nnode + node;
        double acc = 0.0;
        if (self_fixed) {
            if constexpr (TWO) acc = identity ? x[0] : 0.0;
            else acc = x[0];
        } else {
#pragma unroll
            for (int k = 0; k < NB; ++k)
                if ((live >> k) & 1u) acc = fma(coef[k], x[delta[k]], acc);
        }
        if constexpr (TWO) {
            if (b) {
                const double bv = b[col * g.nnode + node];
                acc = residual ? bv - acc : (self_fixed ? acc : acc + bv);
            }
            Y[col * g.nnode + node] = acc;
        } else Y[col * g.nnode + node] = b ? b[col * g.nnode + node] - acc : acc;
    }
}

template <int N, bool TWO>
__global__ void __launch_bounds__(256) k_thermal_diagonal(ModalGrid g, ThermalMatrix K, OnlyTwoTerm<TWO, ThermalCapacity> mb,
                                                          const double *__restrict__ kappa,
                                                          OnlyTwoTerm<TWO, const double *__restrict__> cap,
                                                          const uint8_t *__restrict__ fixed, int invert, double *__restrict__ out) {
    constexpr int NPE = ThermalTraits<N>::NPE;
    int c[N];
    if (!thread_cell<N>(g.ne, 1, c)) return;
    const long long node = flat_index<N>(g.ne, 1, c);
    double d = 0.0;
#pragma unroll
    for (int el = 0; el < NPE; ++el) {
        d = fma(incident_kappa<N>(g, kappa, c, el), K.k[el * NPE + el], d);
        if constexpr (TWO) d = fma(incident_kappa<N>(g, cap, c, el), mb.m[0], d);
    }
    if (fixed && fixed[node]) d = 1.0;
    out[node] = invert ? 1.0 / d : d;
}

template <int N>
__global__ void __launch_bounds__(256) k_thermal_source(ModalGrid g, double share, const double *__restrict__ q,
                                                        const uint8_t *__restrict__ fixed, const double *f_in, double *f_out) {
    constexpr int NPE = ThermalTraits<N>::NPE;
    int c[N];
    if (!thread_cell<N>(g.ne, 1, c)) return;
    const long long node = flat_index<N>(g.ne, 1, c);
    double acc = f_in ? f_in[node] : 0.0;
    if (q) {
#pragma unroll
        for (int el = 0; el < NPE; ++el) acc = fma(incident_kappa<N>(g, q, c, el), share, acc);
    }
    f_out[node] = (fixed && fixed[node]) ? 0.0 : acc;
}

constexpr long long TILE = 64 * 64;

// one thread per stored entry of the nb (bt + 1) tiles, as k_band_assemble (band_spd.hip) has it for the stiffness matrix
template <int N, bool TWO>
__global__ void __launch_bounds__(256) k_thermal_band(ModalGrid g, ThermalMatrix K, OnlyTwoTerm<TWO, ThermalCapacity> mb, long long n,
                                                      long long w, long long nb, int bt, const double *__restrict__ kappa,
                                                      OnlyTwoTerm<TWO, const double *__restrict__> cap,
                                                      const uint8_t *__restrict__ fixed, double *__restrict__ band) {
    constexpr int NPE = ThermalTraits<N>::NPE;
    const long long per_row = (long long) (bt + 1) * TILE;
    for (long long t = (long long) blockIdx.x * 256 + threadIdx.x; t < nb * per_row; t += (long long) gridDim.x * 256) {
        const long long I = t / per_row, d = (t - I * per_row) >> 12;
        const int e = (int) (t & 4095);
        const long long i = I * 64 + (e >> 6), j = (I - d) * 64 + (e & 63);
        double v = 0.0;
        if (i >= n) v = i == j ? 1.0 : 0.0;
        else if (j >= 0 && j <= i && i - j <= w) {
            if (fixed && (fixed[i] || fixed[j])) v = i == j ? 1.0 : 0.0;
            else {
                int xi[3] = {0, 0, 0}, xj[3] = {0, 0, 0}, elo[3] = {0, 0, 0}, ehi[3] = {0, 0, 0};
                long long ri = i, rj = j;
                bool shared = true;
#pragma unroll
                for (int ax = N - 1; ax >= 0; --ax) {
                    const int nn = g.ne[ax] + 1;
                    xi[ax] = (int) (ri % nn); ri /= nn;
                    xj[ax] = (int) (rj % nn); rj /= nn;
                    const int lo = min(xi[ax], xj[ax]), hi = max(xi[ax], xj[ax]);
                    elo[ax] = max(hi - 1, 0);                     // first element that reaches node hi
                    ehi[ax] = min(lo, g.ne[ax] - 1);              // last element that starts at or before node lo
                    shared = shared && elo[ax] <= ehi[ax];
                }
                if (shared)         // the shared elements in ascending element index (in 2-D the third loop runs once)
                    for (int e0 = elo[0]; e0 <= ehi[0]; ++e0)
                        for (int e1 = elo[1]; e1 <= ehi[1]; ++e1)
                            for (int e2 = elo[2]; e2 <= ehi[2]; ++e2) {
                                const int ee[3] = {e0, e1, e2};
                                long long el = 0;
                                int li = 0, lj = 0;
#pragma unroll
                                for (int ax = 0; ax < N; ++ax) {
                                    el = el * g.ne[ax] + ee[ax];
                                    li = 2 * li + xi[ax] - ee[ax];
                                    lj = 2 * lj + xj[ax] - ee[ax];
                                }
                                v = fma(kappa[el], K.k[li * NPE + lj], v);
                                if constexpr (TWO) v = fma(cap[el], mb.m[__popc(li ^ lj)], v);
                            }
            }
        }
        band[(I * (bt + 2) + d) * TILE + e] = v;
    }
}

template <int N>
__global__ void __launch_bounds__(256) k_thermal_gradient(ModalGrid g, ThermalMatrix K, int ncols, ThermalCoef cf,
                                                          const double *__restrict__ dkappa, const double *A, const double *B,
                                                          double *__restrict__ out) {
    constexpr int NPE = ThermalTraits<N>::NPE;
    int ec[N];
    if (!thread_cell<N>(g.ne, 0, ec)) return;
    const long long e = flat_index<N>(g.ne, 0, ec);
    long long nd[NPE];
#pragma unroll
    for (int m = 0; m < NPE; ++m) {
        int c[N];
#pragma unroll
        for (int d = 0; d < N; ++d) c[d] = ec[d] + node_bit<N>(m, d);
        nd[m] = flat_index<N>(g.ne, 1, c);
    }
    double sum = 0.0;
    for (int i = 0; i < ncols; ++i) {
        const double *a = A + i * g.nnode, *b = B + i * g.nnode;
        double be[NPE];
#pragma unroll
        for (int m = 0; m < NPE; ++m) be[m] = b[nd[m]];
        // a_e^T Kc0 b_e one row of Kc0 at a time; rolled, so that the 64 entries are not all held at once (they would not fit the
        // scalar registers beside the column loop), and the row's own value of a comes from memory by a node index formed here
        double q = 0.0;
#pragma unroll 1
        for (int r = 0; r < NPE; ++r) {
            int c[N];
#pragma unroll
            for (int d = 0; d < N; ++d) c[d] = ec[d] + node_bit<N>(r, d);
            double row = 0.0;
#pragma unroll
            for (int m = 0; m < NPE; ++m) row = fma(K.k[r * NPE + m], be[m], row);
            q = fma(a[flat_index<N>(g.ne, 1, c)], row, q);
        }
        sum = fma(cf.c[i], q, sum);
    }
    out[e] = dkappa[e] * sum;
}

template <int N>
__global__ void __launch_bounds__(256) k_thermal_flux(ModalGrid g, ThermalTensor k, const double *__restrict__ kappa,
                                                      const double *__restrict__ T, double *__restrict__ flux) {
    constexpr int NPE = ThermalTraits<N>::NPE;
    int ec[N];
    if (!thread_cell<N>(g.ne, 0, ec)) return;
    const long long e = flat_index<N>(g.ne, 0, ec);
    double grad[N];
#pragma unroll
    for (int d = 0; d < N; ++d) grad[d] = 0.0;
#pragma unroll
    for (int m = 0; m < NPE; ++m) {
        int c[N];
#pragma unroll
        for (int d = 0; d < N; ++d) c[d] = ec[d] + node_bit<N>(m, d);
        const double t = T[flat_index<N>(g.ne, 1, c)];
#pragma unroll
        for (int d = 0; d < N; ++d) grad[d] += node_bit<N>(m, d) ? t : -t;
    }
#pragma unroll
    for (int d = 0; d < N; ++d) grad[d] /= (double) (NPE / 2) * g.h[d];
    const double ke = kappa[e];
#pragma unroll
    for (int a = 0; a < N; ++a) {
        double q = 0.0;
#pragma unroll
        for (int d = 0; d < N; ++d) q = fma(k.k[a * N + d], grad[d], q);
        flux[e * N + a] = -ke * q;
    }
}

__global__ void __launch_bounds__(256) k_thermal_scale(long long n, const double *__restrict__ dinv, const double *__restrict__ r,
                                                       double *__restrict__ z) {
    for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < n; i += (long long) gridDim.x * 256) z[i] = dinv[i] * r[i];
}

__global__ void k_thermal_pcg_guard(double *sc, int stage, int iteration) {
    if (stage == 1 && sc[5] == 0.0 && !(sc[2] > 0.0)) {
        sc[5] = (double) iteration;
        sc[6] = sc[2];
        sc[7] = sc[3];
    }
    if (sc[5] != 0.0) {
        sc[0] = 0.0;
        sc[stage == 1 ? 2 : 1] = 1.0;
    }
}

unsigned blocks_for(long long n) { return (unsigned) std::max<long long>(1, std::min<long long>((n + 255) / 256, 1 << 16)); }

}  // namespace

// `kernel` (a template of N and TWO) in the instantiation for the grid's N; each launcher below has one such line per form, with
// NoCapacity{} where the one-term instantiation has its placeholders
#define THERMAL_LAUNCH(kernel, TWO, N_, ...) \
    do { if ((N_) == 3) kernel<3, TWO> __VA_ARGS__; else kernel<2, TWO> __VA_ARGS__; VFEM_HIP(hipGetLastError()); } while (0)

void launch_thermal_apply(const ModalGrid &g, const ThermalOp &op, const uint8_t *fixed, int identity, int ncols, const double *X,
                          const double *b, int residual, double *Y, hipStream_t s) {
    const dim3 grd = cell_grid(g.N, g.ne, 1);
    const NoCapacity none;
    if (op.cap)
        THERMAL_LAUNCH(k_thermal_apply, true, g.N, <<<grd, cell_block(), 0, s>>>(g, op.K, op.mb, op.kappa, op.cap, fixed, identity, ncols, X, b, residual, Y));
    else {
        if (!identity || (b && !residual)) throw Error("launch_thermal_apply: the one-term form has iota = 1 and takes b for a residual");
        THERMAL_LAUNCH(k_thermal_apply, false, g.N, <<<grd, cell_block(), 0, s>>>(g, op.K, none, op.kappa, none, fixed, none, ncols, X, b, none, Y));
    }
}

void launch_thermal_diagonal(const ModalGrid &g, const ThermalOp &op, const uint8_t *fixed, int invert, double *d, hipStream_t s) {
    const dim3 grd = cell_grid(g.N, g.ne, 1);
    const NoCapacity none;
    if (op.cap) THERMAL_LAUNCH(k_thermal_diagonal, true, g.N, <<<grd, cell_block(), 0, s>>>(g, op.K, op.mb, op.kappa, op.cap, fixed, invert, d));
    else THERMAL_LAUNCH(k_thermal_diagonal, false, g.N, <<<grd, cell_block(), 0, s>>>(g, op.K, none, op.kappa, none, fixed, invert, d));
}

void launch_thermal_source(const ModalGrid &g, const double *q, const uint8_t *fixed, const double *f_in, double *f_out,
                           hipStream_t s) {
    double share = 1.0;
    for (int d = 0; d < g.N; ++d) share *= g.h[d];
    share /= (double) (1 << g.N);
    const dim3 grd = cell_grid(g.N, g.ne, 1);
    if (g.N == 3) k_thermal_source<3><<<grd, cell_block(), 0, s>>>(g, share, q, fixed, f_in, f_out);
    else k_thermal_source<2><<<grd, cell_block(), 0, s>>>(g, share, q, fixed, f_in, f_out);
    VFEM_HIP(hipGetLastError());
}

void launch_thermal_band_assemble(const ModalGrid &g, const ThermalOp &op, const uint8_t *fixed, double *band, hipStream_t s) {
    long long n, w;
    thermal_band_geometry(g, n, w);
    const long long nb = (n + 63) / 64;
    const int bt = (int) ((w + 63) / 64);
    const unsigned blocks = blocks_for(nb * (bt + 1) * TILE);
    const NoCapacity none;
    if (op.cap) THERMAL_LAUNCH(k_thermal_band, true, g.N, <<<blocks, 256, 0, s>>>(g, op.K, op.mb, n, w, nb, bt, op.kappa, op.cap, fixed, band));
    else THERMAL_LAUNCH(k_thermal_band, false, g.N, <<<blocks, 256, 0, s>>>(g, op.K, none, n, w, nb, bt, op.kappa, none, fixed, band));
}

void launch_thermal_gradient(const ModalGrid &g, const ThermalMatrix &K, int ncols, const ThermalCoef &c, const double *dkappa,
                             const double *A, const double *B, double *out, hipStream_t s) {
    const dim3 grd = cell_grid(g.N, g.ne, 0);
    if (g.N == 3) k_thermal_gradient<3><<<grd, cell_block(), 0, s>>>(g, K, ncols, c, dkappa, A, B, out);
    else k_thermal_gradient<2><<<grd, cell_block(), 0, s>>>(g, K, ncols, c, dkappa, A, B, out);
    VFEM_HIP(hipGetLastError());
}

void launch_thermal_flux(const ModalGrid &g, const ThermalTensor &k, const double *kappa, const double *T, double *flux, hipStream_t s) {
    const dim3 grd = cell_grid(g.N, g.ne, 0);
    if (g.N == 3) k_thermal_flux<3><<<grd, cell_block(), 0, s>>>(g, k, kappa, T, flux);
    else k_thermal_flux<2><<<grd, cell_block(), 0, s>>>(g, k, kappa, T, flux);
    VFEM_HIP(hipGetLastError());
}

void launch_thermal_scale(long long n, const double *dinv, const double *r, double *z, hipStream_t s) {
    k_thermal_scale<<<blocks_for(n), 256, 0, s>>>(n, dinv, r, z);
    VFEM_HIP(hipGetLastError());
}

void launch_thermal_pcg_guard(double *sc, int stage, int iteration, hipStream_t s) {
    k_thermal_pcg_guard<<<1, 1, 0, s>>>(sc, stage, iteration);
    VFEM_HIP(hipGetLastError());
}

}  // namespace vfem
