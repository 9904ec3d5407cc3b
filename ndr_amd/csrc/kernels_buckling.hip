// Linearised buckling of a degree-1 grid (buckling.h): the consistent geometric stiffness on a block of vectors, the
// derivative of the modes' Rayleigh quotients with respect to the displacement, and the density gradient of the measure.
//
// All three stream fp64.  Every sum has a fixed order and no kernel uses an atomic: the same bits run to run.  Device pointers need
// 8-byte alignment only (every access is one double).  The table T is read at indices that are the same for every lane: uniform
// loads, no vector register holds an entry of it.
//
// Geometric apply: one thread per NODE (cell_threads.h), all columns.  K_G couples a node to the 3^N nodes around it with ONE scalar
// per pair, the same for all N components.  The thread forms these 3^N scalars once from the 2^N elements around it (mG[e] and the
// element's 2^N N displacements: 2^N 2^N 2^N N multiply-adds, elements in ascending local-node order) and then walks the columns as
// the mass apply of kernels_modal.hip does: 3^N N loads of X and N stores per column.
//
// Adjoint load: one thread per node gathers, over the 2^N elements around it,  mG[e] sum_{n,m} T_j[n][m] S_e[n][m]  for its own N dofs
// j of that element, with  S_e[n][m] = sum_i c_i sum_b phi_i[n][b] phi_i[m][b]  the (symmetric) weighted covariance of the modes on
// the element's nodes: the modes are folded into S once per element, not once per dof.
//
// Gradient: one thread per ELEMENT, the three terms of dJ/drho_e from the same S_e and two kinds of quadratic form in K0.
#include "buckling.h"

#include "cell_threads.h"
#include "device_utils.h"

namespace vfem {

namespace {

template <int N>
struct BucklingTraits {
    static constexpr int NPE = 1 << N;
    static constexpr int KE = N * NPE;
    static constexpr int NB = N == 2 ? 9 : 27;          // nodes coupled to a node
    static constexpr int NS = NPE * (NPE + 1) / 2;      // entries n <= m of a symmetric node matrix
};

// where entry (n, m), n <= m, of a symmetric NPE x NPE matrix is kept
template <int NPE>
__device__ __forceinline__ constexpr int sym_index(int n, int m) { return n * NPE - n * (n - 1) / 2 + (m - n); }

// node index of local node mn of element ec
template <int N>
__device__ __forceinline__ long long element_node(const int *ne, const int (&ec)[N], int mn) {
    int c[N];
#pragma unroll
    for (int d = 0; d < N; ++d) c[d] = ec[d] + node_bit<N>(mn, d);
    return flat_index<N>(ne, 1, c);
}

// S += coef sum_b p[n][b] p[m][b] for n <= m, the element's values p of one mode
template <int N>
__device__ __forceinline__ void add_covariance(double coef, const double (&p)[1 << N][N], double (&S)[BucklingTraits<N>::NS]) {
    constexpr int NPE = 1 << N;
#pragma unroll
    for (int n = 0; n < NPE; ++n)
#pragma unroll
        for (int m = n; m < NPE; ++m) {
            double d = 0.0;
#pragma unroll
            for (int b = 0; b < N; ++b) d = fma(p[n][b], p[m][b], d);
            S[sym_index<NPE>(n, m)] = fma(coef, d, S[sym_index<NPE>(n, m)]);
        }
}

// sum_{n,m} Tj[n][m] S[n][m] for a symmetric table entry Tj [NPE][NPE] (uniform address)
template <int N>
__device__ __forceinline__ double contract(const double *__restrict__ Tj, const double (&S)[BucklingTraits<N>::NS]) {
    constexpr int NPE = 1 << N;
    double s = 0.0;
#pragma unroll
    for (int n = 0; n < NPE; ++n)
#pragma unroll
        for (int m = n; m < NPE; ++m) s = fma((n == m ? 1.0 : 2.0) * Tj[n * NPE + m], S[sym_index<NPE>(n, m)], s);
    return s;
}

// left_e^T K0 right_e: the rows of K0 one node at a time, rolled as in k_modal_gradient; `left` is read from memory again
template <int N>
__device__ __forceinline__ double quadratic_form(const int *ne, const int (&ec)[N], const double *__restrict__ K0,
                                                 const double *__restrict__ left, const double (&right)[1 << N][N]) {
    constexpr int NPE = 1 << N, KE = N * NPE;
    double q = 0.0;
#pragma unroll 1
    for (int mn = 0; mn < NPE; ++mn) {
        const long long nd = element_node<N>(ne, ec, mn);
        const double *rows = K0 + (long long) mn * N * KE;
#pragma unroll
        for (int b = 0; b < N; ++b) {
            double acc = 0.0;
#pragma unroll
            for (int c2 = 0; c2 < KE; ++c2) acc = fma(rows[b * KE + c2], right[c2 / N][c2 % N], acc);
            q = fma(left[N * nd + b], acc, q);
        }
    }
    return q;
}

template <int N>
__global__ void __launch_bounds__(256) k_buckling_geom_apply(ModalGrid g, const double *__restrict__ T, const double *__restrict__ mG,
                                                             const double *__restrict__ u, const uint8_t *__restrict__ mask, int ncols,
                                                             const double *__restrict__ X, double *__restrict__ Y) {
    constexpr int NPE = BucklingTraits<N>::NPE, KE = BucklingTraits<N>::KE, NB = BucklingTraits<N>::NB;
    int c[N];
    if (!thread_cell<N>(g.ne, 1, c)) return;
    const long long node = flat_index<N>(g.ne, 1, c);
    double coef[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) coef[k] = 0.0;
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
        if (in) {
            const double me = mG[flat_index<N>(g.ne, 0, ec)];
            double ue[KE];
#pragma unroll
            for (int mn = 0; mn < NPE; ++mn) {
                const long long nd = element_node<N>(g.ne, ec, mn);
#pragma unroll
                for (int b = 0; b < N; ++b) ue[mn * N + b] = u[N * nd + b];
            }
#pragma unroll
            for (int jn = 0; jn < NPE; ++jn) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < KE; ++j) s = fma(ue[j], T[(j * NPE + el) * NPE + jn], s);
                coef[neighbour_of<N>(el, jn)] = fma(me, s, coef[neighbour_of<N>(el, jn)]);
            }
        }
    }
    long long delta[NB];            // the neighbour's node index minus this one's
    unsigned valid = 0u, fixed[N];
#pragma unroll
    for (int a = 0; a < N; ++a) fixed[a] = 0u;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        bool in = true;
        long long off = 0;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            const int o = neighbour_offset<N>(k, d);
            in = in && c[d] + o >= 0 && c[d] + o <= g.ne[d];
            off = off * (g.ne[d] + 1) + o;
        }
        delta[k] = off;
        if (in) {
            valid |= 1u << k;
            if (mask) {
                const unsigned bits = mask[node + off];
#pragma unroll
                for (int a = 0; a < N; ++a) fixed[a] |= ((bits >> a) & 1u) << k;
            }
        }
    }
    constexpr int SELF = (NB - 1) / 2;
    const long long stride = g.nnode * N;
    for (int col = 0; col < ncols; ++col) {
        const double *__restrict__ x = X + col * stride + node * N;
        double acc[N];
#pragma unroll
        for (int a = 0; a < N; ++a) acc[a] = 0.0;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            if ((valid >> k) & 1u) {
#pragma unroll
                for (int a = 0; a < N; ++a) {
                    const double v = ((fixed[a] >> k) & 1u) ? 0.0 : x[delta[k] * N + a];
                    acc[a] = fma(coef[k], v, acc[a]);
                }
            }
        }
        double *__restrict__ y = Y + col * stride + node * N;
#pragma unroll
        for (int a = 0; a < N; ++a) y[a] = ((fixed[a] >> SELF) & 1u) ? 0.0 : acc[a];
    }
}

template <int N>
__global__ void __launch_bounds__(256) k_buckling_adjoint_load(ModalGrid g, const double *__restrict__ T, const double *__restrict__ mG,
                                                               const uint8_t *__restrict__ mask, int nmodes, BucklingCoef cf,
                                                               const double *__restrict__ Phi, double *__restrict__ a) {
    constexpr int NPE = BucklingTraits<N>::NPE, NS = BucklingTraits<N>::NS;
    int c[N];
    if (!thread_cell<N>(g.ne, 1, c)) return;
    const long long node = flat_index<N>(g.ne, 1, c);
    double acc[N];
#pragma unroll
    for (int b = 0; b < N; ++b) acc[b] = 0.0;
#pragma unroll 1
    for (int el = 0; el < NPE; ++el) {
        int ec[N];
        bool in = true;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            ec[d] = c[d] - node_bit<N>(el, d);
            in = in && ec[d] >= 0 && ec[d] < g.ne[d];
        }
        if (!in) continue;
        double S[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) S[k] = 0.0;
        for (int i = 0; i < nmodes; ++i) {
            const double *__restrict__ phi = Phi + i * g.nnode * N;
            double pe[NPE][N];
#pragma unroll
            for (int mn = 0; mn < NPE; ++mn) {
                const long long nd = element_node<N>(g.ne, ec, mn);
#pragma unroll
                for (int b = 0; b < N; ++b) pe[mn][b] = phi[N * nd + b];
            }
            add_covariance<N>(cf.c[i], pe, S);
        }
        const double me = mG[flat_index<N>(g.ne, 0, ec)];
#pragma unroll
        for (int b = 0; b < N; ++b) acc[b] = fma(me, contract<N>(T + (long long) (el * N + b) * NPE * NPE, S), acc[b]);
    }
    const unsigned bits = mask ? mask[node] : 0u;
#pragma unroll
    for (int b = 0; b < N; ++b) a[N * node + b] = ((bits >> b) & 1u) ? 0.0 : acc[b];
}

template <int N>
__global__ void __launch_bounds__(256) k_buckling_gradient(ModalGrid g, const double *__restrict__ T, const double *__restrict__ K0,
                                                           int nmodes, BucklingCoef cf, const double *__restrict__ dmG,
                                                           const double *__restrict__ dE, const double *__restrict__ u,
                                                           const double *__restrict__ v, const double *__restrict__ Phi,
                                                           double *__restrict__ out) {
    constexpr int NPE = BucklingTraits<N>::NPE, NS = BucklingTraits<N>::NS;
    int ec[N];
    if (!thread_cell<N>(g.ne, 0, ec)) return;
    const long long e = flat_index<N>(g.ne, 0, ec);
    double ue[NPE][N];
#pragma unroll
    for (int mn = 0; mn < NPE; ++mn) {
        const long long nd = element_node<N>(g.ne, ec, mn);
#pragma unroll
        for (int b = 0; b < N; ++b) ue[mn][b] = u[N * nd + b];
    }
    double sK = -quadratic_form<N>(g.ne, ec, K0, v, ue);
    double S[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) S[k] = 0.0;
    for (int i = 0; i < nmodes; ++i) {
        const double *__restrict__ phi = Phi + i * g.nnode * N;
        double pe[NPE][N];
#pragma unroll
        for (int mn = 0; mn < NPE; ++mn) {
            const long long nd = element_node<N>(g.ne, ec, mn);
#pragma unroll
            for (int b = 0; b < N; ++b) pe[mn][b] = phi[N * nd + b];
        }
        add_covariance<N>(cf.c[i], pe, S);
        sK = fma(cf.cK[i], quadratic_form<N>(g.ne, ec, K0, phi, pe), sK);
    }
    // sum_j u_ej (T_j : S), one dof's table at a time (rolled: the dof's displacement comes from memory again)
    double sG = 0.0;
#pragma unroll 1
    for (int mn = 0; mn < NPE; ++mn) {
        const long long nd = element_node<N>(g.ne, ec, mn);
#pragma unroll
        for (int b = 0; b < N; ++b) sG = fma(u[N * nd + b], contract<N>(T + (long long) (mn * N + b) * NPE * NPE, S), sG);
    }
    out[e] = dmG[e] * sG + dE[e] * sK;
}

}  // namespace

void launch_buckling_geom_apply(const ModalGrid &g, const double *T, const double *mG, const double *u, const uint8_t *mask, int ncols,
                                const double *X, double *Y, hipStream_t s) {
    const dim3 grd = cell_grid(g.N, g.ne, 1);
    if (g.N == 3) k_buckling_geom_apply<3><<<grd, cell_block(), 0, s>>>(g, T, mG, u, mask, ncols, X, Y);
    else k_buckling_geom_apply<2><<<grd, cell_block(), 0, s>>>(g, T, mG, u, mask, ncols, X, Y);
    VFEM_HIP(hipGetLastError());
}

void launch_buckling_adjoint_load(const ModalGrid &g, const double *T, const double *mG, const uint8_t *mask, int nmodes,
                                  const BucklingCoef &c, const double *Phi, double *a, hipStream_t s) {
    const dim3 grd = cell_grid(g.N, g.ne, 1);
    if (g.N == 3) k_buckling_adjoint_load<3><<<grd, cell_block(), 0, s>>>(g, T, mG, mask, nmodes, c, Phi, a);
    else k_buckling_adjoint_load<2><<<grd, cell_block(), 0, s>>>(g, T, mG, mask, nmodes, c, Phi, a);
    VFEM_HIP(hipGetLastError());
}

void launch_buckling_gradient(const ModalGrid &g, const double *T, const double *K0, int nmodes, const BucklingCoef &c,
                              const double *dmG, const double *dE, const double *u, const double *v, const double *Phi, double *out,
                              hipStream_t s) {
    const dim3 grd = cell_grid(g.N, g.ne, 0);
    if (g.N == 3) k_buckling_gradient<3><<<grd, cell_block(), 0, s>>>(g, T, K0, nmodes, c, dmG, dE, u, v, Phi, out);
    else k_buckling_gradient<2><<<grd, cell_block(), 0, s>>>(g, T, K0, nmodes, c, dmG, dE, u, v, Phi, out);
    VFEM_HIP(hipGetLastError());
}

}  // namespace vfem
