// Transient heat conduction on a degree-1 grid (transient.h): the two-term operator A(Ka, mb) on a block of nodal
// fields, its diagonal, its band for the direct solver, and the density gradient summed over the steps of a march.
//
// As in kernels_thermal.hip every kernel streams fp64, every sum has a fixed order and none uses an atomic: the same bits run to
// run.  Device pointers need 8-byte alignment only.  Ka (at most 64 doubles) and mb (4 doubles) travel in the kernel arguments.
//
// Apply: k_thermal_apply's form, one thread per NODE and all columns, with the couplings of both terms formed once
// (VFEM_TRANSIENT_COUPLINGS, thermal_device.h).  A fixed node gives iota times its own value; a fixed neighbour is skipped.
//
// Gradient: one thread per ELEMENT marches the steps.  It keeps the 2^N temperatures of the step before in registers, so a row of
// the trajectory is read once per incident element, and the adjoint's value of a matrix row comes from memory by a node index formed
// in the rolled row loop, as k_thermal_gradient has it.
#include "thermal_device.h"
#include "transient.h"

#include <algorithm>

namespace vfem {

namespace {

template <int N>
__global__ void __launch_bounds__(256) k_transient_apply(ModalGrid g, ThermalMatrix K, ThermalCapacity mb, const double *__restrict__ kappa,
                                                         const double *__restrict__ cap, const uint8_t *__restrict__ fixed, int identity,
                                                         int ncols, const double *__restrict__ X, const double *__restrict__ b,
                                                         int residual, double *__restrict__ Y) {
    constexpr int NB = ThermalTraits<N>::NB, SELF = ThermalTraits<N>::SELF;
    int c[N];
    if (!thread_cell<N>(g.ne, 1, c)) return;
    const long long node = flat_index<N>(g.ne, 1, c);
    double coef[NB];
    VFEM_TRANSIENT_COUPLINGS(N, g, K, mb, kappa, cap, c, coef);
    long long delta[NB];            // the neighbour's node index minus this one's
    unsigned live = 0u;             // neighbours inside the grid that are not fixed
    VFEM_THERMAL_LIVE_NEIGHBOURS(N, g, fixed, c, node, delta, live);
    const bool self_fixed = !((live >> SELF) & 1u);
    for (int col = 0; col < ncols; ++col) {
        const double *__restrict__ x = X + col * g.nnode + node;
        double acc = 0.0;
        if (self_fixed) acc = identity ? x[0] : 0.0;
        else {
#pragma unroll
            for (int k = 0; k < NB; ++k)
                if ((live >> k) & 1u) acc = fma(coef[k], x[delta[k]], acc);
        }
        if (b) {
            const double bv = b[col * g.nnode + node];
            acc = residual ? bv - acc : (self_fixed ? acc : acc + bv);
        }
        Y[col * g.nnode + node] = acc;
    }
}

template <int N>
__global__ void __launch_bounds__(256) k_transient_diagonal(ModalGrid g, ThermalMatrix K, ThermalCapacity mb, const double *__restrict__ kappa,
                                                            const double *__restrict__ cap, const uint8_t *__restrict__ fixed, int invert,
                                                            double *__restrict__ out) {
    constexpr int NPE = ThermalTraits<N>::NPE;
    int c[N];
    if (!thread_cell<N>(g.ne, 1, c)) return;
    const long long node = flat_index<N>(g.ne, 1, c);
    double d = 0.0;
#pragma unroll
    for (int el = 0; el < NPE; ++el) {
        d = fma(incident_kappa<N>(g, kappa, c, el), K.k[el * NPE + el], d);
        d = fma(incident_kappa<N>(g, cap, c, el), mb.m[0], d);
    }
    if (fixed && fixed[node]) d = 1.0;
    out[node] = invert ? 1.0 / d : d;
}

constexpr long long TILE = 64 * 64;

// k_thermal_band (kernels_thermal.hip) with the capacity term: one thread per stored entry of the nb (bt + 1) tiles
template <int N>
__global__ void __launch_bounds__(256) k_transient_band(ModalGrid g, ThermalMatrix K, ThermalCapacity mb, long long n, long long w,
                                                        long long nb, int bt, const double *__restrict__ kappa,
                                                        const double *__restrict__ cap, const uint8_t *__restrict__ fixed,
                                                        double *__restrict__ band) {
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
                                v = fma(cap[el], mb.m[__popc(li ^ lj)], v);
                            }
            }
        }
        band[(I * (bt + 2) + d) * TILE + e] = v;
    }
}

template <int N>
__global__ void __launch_bounds__(256) k_transient_gradient(ModalGrid g, ThermalMatrix K, ThermalCapacity mc, long long steps, double dt,
                                                            double theta, const double *__restrict__ dkappa,
                                                            const double *__restrict__ dcap, const double *__restrict__ T,
                                                            const double *__restrict__ Lam, double *__restrict__ out) {
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
    double prev[NPE];               // the element's temperatures of the step before
#pragma unroll
    for (int m = 0; m < NPE; ++m) prev[m] = T[nd[m]];
    const double other = 1.0 - theta;
    double sum_c = 0.0, sum_k = 0.0;
    for (long long n = 1; n <= steps; ++n) {
        const double *__restrict__ t = T + n * g.nnode, *__restrict__ lam = Lam + n * g.nnode;
        double rate[NPE], mean[NPE];            // T^n - T^(n-1), and theta T^n + (1 - theta) T^(n-1)
#pragma unroll
        for (int m = 0; m < NPE; ++m) {
            const double now = t[nd[m]];
            rate[m] = now - prev[m];
            mean[m] = fma(theta, now, other * prev[m]);
            prev[m] = now;
        }
        // one row of both matrices at a time; rolled, so that the 64 entries of K are not all held at once
        double qc = 0.0, qk = 0.0;
#pragma unroll 1
        for (int r = 0; r < NPE; ++r) {
            int c[N];
#pragma unroll
            for (int d = 0; d < N; ++d) c[d] = ec[d] + node_bit<N>(r, d);
            double row_c = 0.0, row_k = 0.0;
#pragma unroll
            for (int m = 0; m < NPE; ++m) {
                row_c = fma(mc.m[__popc(r ^ m)], rate[m], row_c);
                row_k = fma(K.k[r * NPE + m], mean[m], row_k);
            }
            const double l = lam[flat_index<N>(g.ne, 1, c)];
            qc = fma(l, row_c, qc);
            qk = fma(l, row_k, qk);
        }
        sum_c += qc;
        sum_k += qk;
    }
    out[e] = -fma(dcap[e] / dt, sum_c, dkappa[e] * sum_k);
}

unsigned blocks_for(long long n) { return (unsigned) std::max<long long>(1, std::min<long long>((n + 255) / 256, 1 << 16)); }

}  // namespace

void launch_transient_apply(const ModalGrid &g, const ThermalMatrix &Ka, const ThermalCapacity &mb, const double *kappa, const double *cap,
                            const uint8_t *fixed, int identity, int ncols, const double *X, const double *b, int residual, double *Y,
                            hipStream_t s) {
    const dim3 grd = cell_grid(g.N, g.ne, 1);
    if (g.N == 3) k_transient_apply<3><<<grd, cell_block(), 0, s>>>(g, Ka, mb, kappa, cap, fixed, identity, ncols, X, b, residual, Y);
    else k_transient_apply<2><<<grd, cell_block(), 0, s>>>(g, Ka, mb, kappa, cap, fixed, identity, ncols, X, b, residual, Y);
    VFEM_HIP(hipGetLastError());
}

void launch_transient_diagonal(const ModalGrid &g, const ThermalMatrix &Ka, const ThermalCapacity &mb, const double *kappa,
                               const double *cap, const uint8_t *fixed, int invert, double *d, hipStream_t s) {
    const dim3 grd = cell_grid(g.N, g.ne, 1);
    if (g.N == 3) k_transient_diagonal<3><<<grd, cell_block(), 0, s>>>(g, Ka, mb, kappa, cap, fixed, invert, d);
    else k_transient_diagonal<2><<<grd, cell_block(), 0, s>>>(g, Ka, mb, kappa, cap, fixed, invert, d);
    VFEM_HIP(hipGetLastError());
}

void launch_transient_band_assemble(const ModalGrid &g, const ThermalMatrix &Ka, const ThermalCapacity &mb, const double *kappa,
                                    const double *cap, const uint8_t *fixed, double *band, hipStream_t s) {
    long long n, w;
    thermal_band_geometry(g, n, w);
    const long long nb = (n + 63) / 64;
    const int bt = (int) ((w + 63) / 64);
    const unsigned blocks = blocks_for(nb * (bt + 1) * TILE);
    if (g.N == 3) k_transient_band<3><<<blocks, 256, 0, s>>>(g, Ka, mb, n, w, nb, bt, kappa, cap, fixed, band);
    else k_transient_band<2><<<blocks, 256, 0, s>>>(g, Ka, mb, n, w, nb, bt, kappa, cap, fixed, band);
    VFEM_HIP(hipGetLastError());
}

void launch_transient_gradient(const ModalGrid &g, const ThermalMatrix &K, const ThermalCapacity &m, long long steps, double dt,
                               double theta, const double *dkappa, const double *dcap, const double *T, const double *Lam, double *out,
                               hipStream_t s) {
    const dim3 grd = cell_grid(g.N, g.ne, 0);
    if (g.N == 3) k_transient_gradient<3><<<grd, cell_block(), 0, s>>>(g, K, m, steps, dt, theta, dkappa, dcap, T, Lam, out);
    else k_transient_gradient<2><<<grd, cell_block(), 0, s>>>(g, K, m, steps, dt, theta, dkappa, dcap, T, Lam, out);
    VFEM_HIP(hipGetLastError());
}

}  // namespace vfem
