// Transient heat conduction on a degree-1 grid (transient.h): the density gradient summed over the steps of a march.  The
// two-term operator of a step, its diagonal and its band are instantiations of the kernels of kernels_thermal.hip.
//
// As there the kernel streams fp64, every sum has a fixed order and nothing uses an atomic: the same bits run to run.  Device
// pointers need 8-byte alignment only.  K (at most 64 doubles) and m (4 doubles) travel in the kernel arguments.
//
// Gradient: one thread per ELEMENT marches the steps.  It keeps the 2^N temperatures of the step before in registers, so a row of
// the trajectory is read once per incident element, and the adjoint's value of a matrix row comes from memory by a node index formed
// in the rolled row loop, as k_thermal_gradient has it.
#include "thermal_device.h"
#include "transient.h"

namespace vfem {

namespace {

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

}  // namespace

void launch_transient_gradient(const ModalGrid &g, const ThermalMatrix &K, const ThermalCapacity &m, long long steps, double dt,
                               double theta, const double *dkappa, const double *dcap, const double *T, const double *Lam, double *out,
                               hipStream_t s) {
    const dim3 grd = cell_grid(g.N, g.ne, 0);
    if (g.N == 3) k_transient_gradient<3><<<grd, cell_block(), 0, s>>>(g, K, m, steps, dt, theta, dkappa, dcap, T, Lam, out);
    else k_transient_gradient<2><<<grd, cell_block(), 0, s>>>(g, K, m, steps, dt, theta, dkappa, dcap, T, Lam, out);
    VFEM_HIP(hipGetLastError());
}

}  // namespace vfem
