// Thermo-elastic coupling of a degree-1 grid (thermoelastic.h): the load of a temperature field interpolated inside
// the elements, its transpose (the source of the thermal adjoint), and the coupling's term of the density gradient.
//
// All three work on fp64 streams.  Every sum has a fixed order and no kernel uses an atomic: the same bits
// run to run.  Device pointers need 8-byte alignment only (every access is one double).  G is row-major [ke = N 2^N][npe = 2^N],
// the local node order of K0.
//
// Load: one thread per NODE (cell_threads.h).  It loads the 3^N temperatures around it once and takes off T_ref.  In element `el` of
// the 2^N around it the node is local node `el`, so it takes the N rows (el, a) of G times that element's temperatures (columns
// ascending) times that element's modulus, elements in ascending `el`.  G travels in the kernel arguments (192 doubles in 3-D) and
// is read by uniform loads.  The thread writes its own node only, so the output may be the input.
//
// Adjoint source: one thread per NODE, the transpose.  Per case it loads the N 3^N displacements around the node once; in element
// `el` it takes column `el` of G against that element's displacements, rows (n, a) ascending, times the element's modulus; cases
// ascending.  The moduli of the 2^N elements are read once for all cases.  The G of every case is a table in device memory, read by
// uniform loads (the case loop is rolled: the table's address is uniform, the offsets are constants).
//
// Gradient: one thread per ELEMENT.  It loads the element's 2^N temperatures once; per case it loads the element's N 2^N
// displacements once and forms u_e^T G theta_e, rows ascending, the columns ascending within a row, in twice the working precision
// (Sum2 below), and rounds once at the end.
#include "thermoelastic.h"

#include "cell_threads.h"

namespace vfem {

namespace {

// A node's surroundings without a 64-bit multiplication per neighbour: the node's own flat index and that of the element it is
// local node 0 of, the uniform strides of both numberings, and on which sides of every axis the grid goes on.
template <int N>
struct Around {
    long long node, elem;           // elem: the element with this node as its lowest corner (its index formula; it may lie outside)
    int nstride[N], estride[N];     // uniform: last axis 1
    bool lo[N], hi[N];              // a node before / after this one along axis d; hi also: an element starts here

    __device__ __forceinline__ Around(const int *ne, const int (&c)[N]) {
        node = flat_index<N>(ne, 1, c);
        elem = flat_index<N>(ne, 0, c);
        nstride[N - 1] = estride[N - 1] = 1;
#pragma unroll
        for (int d = N - 2; d >= 0; --d) {
            nstride[d] = nstride[d + 1] * (ne[d + 1] + 1);
            estride[d] = estride[d + 1] * ne[d + 1];
        }
#pragma unroll
        for (int d = 0; d < N; ++d) {
            lo[d] = c[d] > 0;
            hi[d] = c[d] < ne[d];
        }
    }
    // neighbour k of the 3^N: flat index, or -1 outside the grid
    __device__ __forceinline__ long long neighbour(int k) const {
        bool in = true;
        long long off = 0;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            const int o = neighbour_offset<N>(k, d);
            in = in && (o < 0 ? lo[d] : o > 0 ? hi[d] : true);
            off += (long long) o * nstride[d];
        }
        return in ? node + off : -1;
    }
    // element `el` of the 2^N around the node (the node is its local node `el`): flat index, or -1 outside the grid
    __device__ __forceinline__ long long element(int el) const {
        bool in = true;
        long long off = 0;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            const int bit = node_bit<N>(el, d);
            in = in && (bit ? lo[d] : hi[d]);
            off += (long long) bit * estride[d];
        }
        return in ? elem - off : -1;
    }
};

template <int N>
__global__ void __launch_bounds__(256) k_te_load(ModalGrid g, TeMatrix G, double tref, const double *__restrict__ E,
                                                 const double *__restrict__ T, const uint8_t *__restrict__ mask, const double *f_in,
                                                 double *f_out) {
    constexpr int NPE = 1 << N, NB = N == 3 ? 27 : 9;
    int c[N];
    if (!thread_cell<N>(g.ne, 1, c)) return;
    const Around<N> ar(g.ne, c);
    const long long node = ar.node;
    double th[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const long long nd = ar.neighbour(k);
        th[k] = nd >= 0 ? T[nd] - tref : 0.0;           // (a node outside the grid belongs to no element taken below)
    }
    double acc[N];
#pragma unroll
    for (int a = 0; a < N; ++a) acc[a] = f_in ? f_in[node * N + a] : 0.0;
#pragma unroll
    for (int el = 0; el < NPE; ++el) {
        const long long e = ar.element(el);
        if (e < 0) continue;
        const double Ee = E[e];
#pragma unroll
        for (int a = 0; a < N; ++a) {
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < NPE; ++m) s = fma(G.G[(el * N + a) * NPE + m], th[neighbour_of<N>(el, m)], s);
            acc[a] = fma(Ee, s, acc[a]);
        }
    }
    const unsigned bits = mask ? mask[node] : 0u;
#pragma unroll
    for (int a = 0; a < N; ++a) f_out[node * N + a] = ((bits >> a) & 1u) ? 0.0 : acc[a];
}

template <int N>
__global__ void __launch_bounds__(256) k_te_adjoint_source(ModalGrid g, int ncases, const double *__restrict__ G, TeCoef cf,
                                                           const double *__restrict__ E, const double *__restrict__ U,
                                                           const uint8_t *__restrict__ fixed, double *__restrict__ q) {
    constexpr int NPE = 1 << N, KE = N * NPE, NB = N == 3 ? 27 : 9;
    int c[N];
    if (!thread_cell<N>(g.ne, 1, c)) return;
    const Around<N> ar(g.ne, c);
    const long long node = ar.node;
    if (fixed && fixed[node]) {
        q[node] = 0.0;
        return;
    }
    int nb[NB];                                      // (a grid has at most 2^31 nodes, grid_args.h)
#pragma unroll
    for (int k = 0; k < NB; ++k) nb[k] = (int) ar.neighbour(k);
    double Ee[NPE];
    bool in[NPE];
#pragma unroll
    for (int el = 0; el < NPE; ++el) {
        const long long e = ar.element(el);
        in[el] = e >= 0;
        Ee[el] = in[el] ? E[e] : 0.0;
    }
    double out = 0.0;
#pragma unroll 1
    for (int i = 0; i < ncases; ++i) {
        const double *__restrict__ u = U + i * g.nnode * N;
        const double *__restrict__ Gi = G + i * (KE * NPE);
        double un[NB][N];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
#pragma unroll
            for (int a = 0; a < N; ++a) un[k][a] = nb[k] >= 0 ? u[(long long) nb[k] * N + a] : 0.0;
        }
        double r = 0.0;
#pragma unroll
        for (int el = 0; el < NPE; ++el) {
            if (!in[el]) continue;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < KE; ++k) s = fma(Gi[k * NPE + el], un[neighbour_of<N>(el, k / N)][k % N], s);
            r = fma(Ee[el], s, r);
        }
        out = fma(cf.a[i], r, out);
    }
    q[node] = out;
}

// Sums of products in twice the working precision (Ogita, Rump and Oishi's Dot2: the exact error of every product, by a fused
// multiply-add, and of every addition, by Knuth's TwoSum, is summed beside the result).  The gradient uses it: u_e^T G theta_e over
// cases whose coefficients and terms have either sign cancels, and one element's entry is one number, so what is written is the
// rounded value of the sum and no summation order shows in it.  The intrinsics keep the compiler from contracting or
// reassociating the error terms away.
__device__ __forceinline__ void two_sum(double a, double b, double &s, double &err) {
    s = __dadd_rn(a, b);
    const double bb = __dadd_rn(s, -a);
    err = __dadd_rn(__dadd_rn(a, -__dadd_rn(s, -bb)), __dadd_rn(b, -bb));
}

struct Sum2 {
    double hi = 0.0, lo = 0.0;
    // += a (bh + bl), |bl| a rounding of bh
    __device__ __forceinline__ void add(double a, double bh, double bl) {
        const double p = __dmul_rn(a, bh);
        const double pe = __fma_rn(a, bh, -p);
        double t, te;
        two_sum(hi, p, t, te);
        hi = t;
        lo = __dadd_rn(lo, __dadd_rn(te, __fma_rn(a, bl, pe)));
    }
    // the sum as a leading part and its remainder
    __device__ __forceinline__ void value(double &h, double &l) const {
        h = __dadd_rn(hi, lo);
        l = __dadd_rn(lo, -__dadd_rn(h, -hi));
    }
};

template <int N>
__global__ void __launch_bounds__(256) k_te_gradient(ModalGrid g, int ncases, const double *__restrict__ G, TeCoef cf,
                                                     const double *__restrict__ dE, const double *__restrict__ T,
                                                     const double *__restrict__ U, const double *g_in, double *g_out) {
    constexpr int NPE = 1 << N, KE = N * NPE;
    int ec[N];
    if (!thread_cell<N>(g.ne, 0, ec)) return;
    const long long e = flat_index<N>(g.ne, 0, ec);
    const long long base = flat_index<N>(g.ne, 1, ec);         // the element's lowest corner; its other nodes by uniform strides
    int nstride[N];
    nstride[N - 1] = 1;
#pragma unroll
    for (int d = N - 2; d >= 0; --d) nstride[d] = nstride[d + 1] * (g.ne[d + 1] + 1);
    long long nd[NPE];
    double Te[NPE];
#pragma unroll
    for (int m = 0; m < NPE; ++m) {
        long long off = 0;
#pragma unroll
        for (int d = 0; d < N; ++d) off += (long long) node_bit<N>(m, d) * nstride[d];
        nd[m] = base + off;
        Te[m] = T[nd[m]];
    }
    Sum2 sum;
#pragma unroll 1
    for (int i = 0; i < ncases; ++i) {
        const double *__restrict__ u = U + i * g.nnode * N;
        const double *__restrict__ Gi = G + i * (KE * NPE);
        const double tref = cf.tref[i];
        double th[NPE], tl[NPE];                // theta = T - T_ref without its rounding: th + tl exactly
#pragma unroll
        for (int m = 0; m < NPE; ++m) two_sum(Te[m], -tref, th[m], tl[m]);
        double ue[KE];
#pragma unroll
        for (int k = 0; k < KE; ++k) ue[k] = u[nd[k / N] * N + k % N];
        Sum2 qi;
#pragma unroll
        for (int k = 0; k < KE; ++k) {
            Sum2 row;
#pragma unroll
            for (int m = 0; m < NPE; ++m) row.add(Gi[k * NPE + m], th[m], tl[m]);
            double sh, sl;
            row.value(sh, sl);
            qi.add(ue[k], sh, sl);
        }
        double qh, ql;
        qi.value(qh, ql);
        sum.add(cf.a[i], qh, ql);
    }
    double sh, sl;
    sum.value(sh, sl);
    Sum2 r;
    r.hi = g_in ? g_in[e] : 0.0;
    r.add(dE[e], sh, sl);
    g_out[e] = __dadd_rn(r.hi, r.lo);
}

}  // namespace

void launch_te_load(const ModalGrid &g, const TeMatrix &G, double tref, const double *E, const double *T, const uint8_t *mask,
                    const double *f_in, double *f_out, hipStream_t s) {
    const dim3 grd = cell_grid(g.N, g.ne, 1);
    if (g.N == 3) k_te_load<3><<<grd, cell_block(), 0, s>>>(g, G, tref, E, T, mask, f_in, f_out);
    else k_te_load<2><<<grd, cell_block(), 0, s>>>(g, G, tref, E, T, mask, f_in, f_out);
    VFEM_HIP(hipGetLastError());
}

void launch_te_adjoint_source(const ModalGrid &g, int ncases, const double *G, const TeCoef &c, const double *E, const double *U,
                              const uint8_t *fixed, double *q, hipStream_t s) {
    const dim3 grd = cell_grid(g.N, g.ne, 1);
    if (g.N == 3) k_te_adjoint_source<3><<<grd, cell_block(), 0, s>>>(g, ncases, G, c, E, U, fixed, q);
    else k_te_adjoint_source<2><<<grd, cell_block(), 0, s>>>(g, ncases, G, c, E, U, fixed, q);
    VFEM_HIP(hipGetLastError());
}

void launch_te_gradient(const ModalGrid &g, int ncases, const double *G, const TeCoef &c, const double *dE, const double *T,
                        const double *U, const double *g_in, double *g_out, hipStream_t s) {
    const dim3 grd = cell_grid(g.N, g.ne, 0);
    if (g.N == 3) k_te_gradient<3><<<grd, cell_block(), 0, s>>>(g, ncases, G, c, dE, T, U, g_in, g_out);
    else k_te_gradient<2><<<grd, cell_block(), 0, s>>>(g, ncases, G, c, dE, T, U, g_in, g_out);
    VFEM_HIP(hipGetLastError());
}

}  // namespace vfem
