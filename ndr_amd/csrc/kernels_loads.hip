// Load cases of a degree-1 grid (loads.h): the assembly of a design-dependent load (self-weight, eigenstrain) and the
// density gradient of a weighted sum of compliances over up to LOADS_MAX_CASES load cases.
//
// Both stream fp64 and do little arithmetic per byte.  Every sum has a fixed order and no kernel uses an atomic: the same bits run
// to run.  Device pointers need 8-byte alignment only (every access is one double).
//
// Assemble: one thread per NODE (cell_threads.h).  In element `el` of the 2^N around it the node is local node `el`, so it takes the
// N entries (el, a) of each pattern times that element's multiplier, elements in ascending `el`, the body-force term before the
// eigenstrain term.  The two patterns travel in the kernel arguments (48 doubles) and are read by uniform loads.  The thread reads
// and writes its own node only, so the output may be the input.
//
// Gradient: one thread per ELEMENT.  Per case it loads the element's 2^N N displacements once, forms u_e^T K0 u_e rolled over the
// node rows of K0 (k_modal_gradient's form: the rows of K0 are not all in flight at once) and the two pattern products, and adds
// them to three sums; dE and dm are read once, g is written once.  K0 and the patterns are a table in device memory, read by
// uniform loads.
#include "loads.h"

#include "cell_threads.h"

namespace vfem {

namespace {

template <int N>
__global__ void __launch_bounds__(256) k_loads_assemble(ModalGrid g, LoadPatterns p, const double *__restrict__ m,
                                                        const double *__restrict__ E, const uint8_t *__restrict__ mask,
                                                        const double *f_in, double *f_out) {
    constexpr int NPE = 1 << N;
    int c[N];
    if (!thread_cell<N>(g.ne, 1, c)) return;
    const long long node = flat_index<N>(g.ne, 1, c);
    double acc[N];
#pragma unroll
    for (int a = 0; a < N; ++a) acc[a] = f_in ? f_in[node * N + a] : 0.0;
    // in element `el` this node is local node `el`: the element sits one step back along every axis whose bit is set
#pragma unroll
    for (int el = 0; el < NPE; ++el) {
        int ec[N];
        bool in = true;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            ec[d] = c[d] - node_bit<N>(el, d);
            in = in && ec[d] >= 0 && ec[d] < g.ne[d];
        }
        if (!in) continue;
        const long long e = flat_index<N>(g.ne, 0, ec);
        if (m) {
            const double me = m[e];
#pragma unroll
            for (int a = 0; a < N; ++a) acc[a] = fma(me, p.Lb[el * N + a], acc[a]);
        }
        if (E) {
            const double Ee = E[e];
#pragma unroll
            for (int a = 0; a < N; ++a) acc[a] = fma(Ee, p.Lt[el * N + a], acc[a]);
        }
    }
    const unsigned bits = mask ? mask[node] : 0u;
#pragma unroll
    for (int a = 0; a < N; ++a) f_out[node * N + a] = ((bits >> a) & 1u) ? 0.0 : acc[a];
}

template <int N>
__global__ void __launch_bounds__(256) k_loads_gradient(ModalGrid g, int ncases, const double *__restrict__ K0,
                                                        const double *__restrict__ Lb, const double *__restrict__ Lt, LoadCoef cf,
                                                        const double *__restrict__ dE, const double *__restrict__ dm,
                                                        const double *__restrict__ U, double *__restrict__ out) {
    constexpr int NPE = 1 << N, KE = N * NPE;
    int ec[N];
    if (!thread_cell<N>(g.ne, 0, ec)) return;
    const long long e = flat_index<N>(g.ne, 0, ec);
    double sK = 0.0, sB = 0.0, sT = 0.0;
    for (int i = 0; i < ncases; ++i) {
        const double *__restrict__ u = U + i * g.nnode * N;
        double ue[NPE][N];
#pragma unroll
        for (int mn = 0; mn < NPE; ++mn) {
            int c[N];
#pragma unroll
            for (int d = 0; d < N; ++d) c[d] = ec[d] + node_bit<N>(mn, d);
            const long long nd = flat_index<N>(g.ne, 1, c);
#pragma unroll
            for (int b = 0; b < N; ++b) ue[mn][b] = u[N * nd + b];
        }
        // u_e^T K0 u_e, one node's rows at a time; rolled, so the node's own values come from memory again (a cache hit) instead of
        // a register indexed at run time
        double qK = 0.0;
#pragma unroll 1
        for (int mn = 0; mn < NPE; ++mn) {
            int c[N];
#pragma unroll
            for (int d = 0; d < N; ++d) c[d] = ec[d] + node_bit<N>(mn, d);
            const long long nd = flat_index<N>(g.ne, 1, c);
            const double *rows = K0 + (long long) mn * N * KE;
#pragma unroll
            for (int b = 0; b < N; ++b) {
                double acc = 0.0;
#pragma unroll
                for (int c2 = 0; c2 < KE; ++c2) acc = fma(rows[b * KE + c2], ue[c2 / N][c2 % N], acc);
                qK = fma(u[N * nd + b], acc, qK);
            }
        }
        sK = fma(cf.cK[i], qK, sK);
        if (Lb) {
            const double *pat = Lb + i * KE;
            double q = 0.0;
#pragma unroll
            for (int k = 0; k < KE; ++k) q = fma(pat[k], ue[k / N][k % N], q);
            sB = fma(cf.cB[i], q, sB);
        }
        if (Lt) {
            const double *pat = Lt + i * KE;
            double q = 0.0;
#pragma unroll
            for (int k = 0; k < KE; ++k) q = fma(pat[k], ue[k / N][k % N], q);
            sT = fma(cf.cT[i], q, sT);
        }
    }
    const double de = dE[e];
    double r = de * sK;
    if (Lb) r = fma(dm[e], sB, r);
    if (Lt) r = fma(de, sT, r);
    out[e] = r;
}

}  // namespace

void launch_loads_assemble(const ModalGrid &g, const LoadPatterns &p, const double *m, const double *E, const uint8_t *mask,
                           const double *f_in, double *f_out, hipStream_t s) {
    const dim3 grd = cell_grid(g.N, g.ne, 1);
    if (g.N == 3) k_loads_assemble<3><<<grd, cell_block(), 0, s>>>(g, p, m, E, mask, f_in, f_out);
    else k_loads_assemble<2><<<grd, cell_block(), 0, s>>>(g, p, m, E, mask, f_in, f_out);
    VFEM_HIP(hipGetLastError());
}

void launch_loads_gradient(const ModalGrid &g, int ncases, const double *K0, const double *Lb, const double *Lt, const LoadCoef &c,
                           const double *dE, const double *dm, const double *U, double *out, hipStream_t s) {
    const dim3 grd = cell_grid(g.N, g.ne, 0);
    if (g.N == 3) k_loads_gradient<3><<<grd, cell_block(), 0, s>>>(g, ncases, K0, Lb, Lt, c, dE, dm, U, out);
    else k_loads_gradient<2><<<grd, cell_block(), 0, s>>>(g, ncases, K0, Lb, Lt, c, dE, dm, U, out);
    VFEM_HIP(hipGetLastError());
}

}  // namespace vfem
