// Natural frequencies of a degree-1 grid (modal.h): the consistent mass operator on a block of vectors, the two dense
// operations of a block eigensolver on tall blocks (Gram matrix, linear combination), the projection onto the free components and
// the density gradient of a combination of Rayleigh quotients.
//
// All of them stream fp64 and do little arithmetic per byte.  Every sum has a fixed order and no kernel uses an atomic: the same
// bits run to run.  Device pointers need 8-byte alignment only (every access is one double).
//
// Mass apply: one thread per NODE (cell_threads.h), all columns.  M couples a node to the 3^N nodes around it, and the coupling of
// the pair (node, node + o) is  w(o) sum of m[e] over the elements that hold both,  w(o) = prod_d (h_d / 6) (o_d == 0 ? 2 : 1).  The
// thread forms these 3^N coefficients once from its 2^N multipliers (added in ascending local-node order) and then walks the
// columns: 3^N N loads of X and N stores per column, the multipliers and the mask are not read again.  (A thread per component of
// a node, so that a wave reads consecutive doubles instead of one double every 8 N bytes, was tried and measured slower: 5.19 ms
// against 2.94 ms for six columns on 256 x 256 x 128, DESIGN 3.13: three times the threads repeat the node's set-up.)
//
// Gram: grid (GRAM_BLOCKS, tiles).  A thread keeps a T x T tile of sums (T = 1, 4 or GRAM_TILE, the smallest that covers the larger
// block, so that a single column costs no idle loads) over the rows  blockIdx.x 256 + threadIdx.x + k GRAM_BLOCKS 256;  the block
// adds its 256 threads (shuffles, then the four waves in order) and stores one partial per entry;  k_block_gram_finish adds the
// GRAM_BLOCKS partials of an entry.  The longest chain of additions behind an entry has  ceil(n / (GRAM_BLOCKS 256)) + 22  terms.
//
// Combine: one thread per row, COMBINE_TILE output columns per launch; the coefficients travel in the kernel arguments.
#include "modal.h"

#include "cell_threads.h"
#include "device_utils.h"

namespace vfem {

namespace {

template <int N>
struct ModalTraits {
    static constexpr int NPE = 1 << N;
    static constexpr int KE = N * NPE;
    static constexpr int NB = N == 2 ? 9 : 27;          // nodes coupled to a node
};

template <int N>
__global__ void __launch_bounds__(256) k_modal_mass_apply(ModalGrid g, const double *__restrict__ m, const uint8_t *__restrict__ mask,
                                                          int ncols, const double *__restrict__ X, double *__restrict__ Y) {
    constexpr int NPE = ModalTraits<N>::NPE, NB = ModalTraits<N>::NB;
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
        const double me = in ? m[flat_index<N>(g.ne, 0, ec)] : 0.0;
#pragma unroll
        for (int j = 0; j < NPE; ++j) coef[neighbour_of<N>(el, j)] += me;
    }
    double vol = 1.0;
#pragma unroll
    for (int d = 0; d < N; ++d) vol *= g.h[d] / 6.0;
    long long delta[NB];            // the neighbour's node index minus this one's
    unsigned valid = 0u, fixed[N];
#pragma unroll
    for (int a = 0; a < N; ++a) fixed[a] = 0u;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        bool in = true;
        long long off = 0;
        int same = 0;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            const int o = neighbour_offset<N>(k, d);
            in = in && c[d] + o >= 0 && c[d] + o <= g.ne[d];
            off = off * (g.ne[d] + 1) + o;
            same += o == 0;
        }
        delta[k] = off;
        coef[k] *= vol * (double) (1 << same);
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

__global__ void __launch_bounds__(256) k_modal_project(long long nnode, int N, const uint8_t *__restrict__ mask, int ncols,
                                                       double *__restrict__ X) {
    const long long node = (long long) blockIdx.x * 256 + threadIdx.x;
    if (node >= nnode) return;
    const unsigned bits = mask[node];
    if (!bits) return;
    for (int col = 0; col < ncols; ++col)
        for (int a = 0; a < N; ++a)
            if ((bits >> a) & 1u) X[(col * nnode + node) * N + a] = 0.0;
}

// ---- Gram matrix: per-workgroup partials, one finishing kernel ----

template <int T>
__global__ void __launch_bounds__(256) k_block_gram_partial(long long n, int ka, const double *__restrict__ A, int kb,
                                                            const double *__restrict__ B, double *__restrict__ partial) {
    __shared__ double sh[4][T * T];
    const int tiles_j = (kb + T - 1) / T;
    const int i0 = (int) (blockIdx.y / tiles_j) * T, j0 = (int) (blockIdx.y % tiles_j) * T;
    // a column past the block's last one reads the last one again: its sums are not stored
    const double *a[T], *b[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        a[t] = A + (long long) min(i0 + t, ka - 1) * n;
        b[t] = B + (long long) min(j0 + t, kb - 1) * n;
    }
    double acc[T][T];
#pragma unroll
    for (int p = 0; p < T; ++p)
#pragma unroll
        for (int q = 0; q < T; ++q) acc[p][q] = 0.0;
    for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < n; i += (long long) GRAM_BLOCKS * 256) {
        double av[T], bv[T];
#pragma unroll
        for (int t = 0; t < T; ++t) { av[t] = a[t][i]; bv[t] = b[t][i]; }
#pragma unroll
        for (int p = 0; p < T; ++p)
#pragma unroll
            for (int q = 0; q < T; ++q) acc[p][q] = fma(av[p], bv[q], acc[p][q]);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int p = 0; p < T; ++p)
#pragma unroll
        for (int q = 0; q < T; ++q) {
            const double v = wave_sum(acc[p][q]);
            if (lane == 0) sh[w][p * T + q] = v;
        }
    __syncthreads();
    if (threadIdx.x < T * T) {
        const int t = threadIdx.x, i = i0 + t / T, j = j0 + t % T;
        if (i < ka && j < kb) partial[(long long) blockIdx.x * ka * kb + i * kb + j] = sh[0][t] + sh[1][t] + sh[2][t] + sh[3][t];
    }
}

__global__ void __launch_bounds__(256) k_block_gram_finish(int entries, const double *__restrict__ partial, double *__restrict__ G) {
    __shared__ double sh[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < GRAM_BLOCKS; i += 256) acc += partial[(long long) i * entries + blockIdx.x];
    const double t = block_sum_256(acc, sh);
    if (threadIdx.x == 0) G[blockIdx.x] = t;
}

template <int T>
void gram_tiles(long long n, int ka, const double *A, int kb, const double *B, double *partial, hipStream_t s) {
    const dim3 grd(GRAM_BLOCKS, (unsigned) (((ka + T - 1) / T) * ((kb + T - 1) / T)));
    k_block_gram_partial<T><<<grd, 256, 0, s>>>(n, ka, A, kb, B, partial);
}

// ---- linear combination ----

__global__ void __launch_bounds__(256) k_block_combine(long long n, int kin, int jn, const double *__restrict__ A, CombineCoef cf,
                                                       double *__restrict__ B) {
    for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < n; i += (long long) gridDim.x * 256) {
        double acc[COMBINE_TILE];
#pragma unroll
        for (int j = 0; j < COMBINE_TILE; ++j) acc[j] = 0.0;
        for (int r = 0; r < kin; ++r) {
            const double a = A[r * n + i];
#pragma unroll
            for (int j = 0; j < COMBINE_TILE; ++j) acc[j] = fma(cf.c[r][j], a, acc[j]);
        }
#pragma unroll
        for (int j = 0; j < COMBINE_TILE; ++j)
            if (j < jn) B[j * n + i] = acc[j];
    }
}

// ---- the density gradient ----

template <int N>
__global__ void __launch_bounds__(256) k_modal_gradient(ModalGrid g, int nmodes, const double *__restrict__ K0, ModalCoef cf,
                                                        const double *__restrict__ dE, const double *__restrict__ dm,
                                                        const double *__restrict__ Phi, double *__restrict__ out) {
    constexpr int NPE = ModalTraits<N>::NPE, KE = ModalTraits<N>::KE;
    int ec[N];
    if (!thread_cell<N>(g.ne, 0, ec)) return;
    const long long e = flat_index<N>(g.ne, 0, ec);
    double vol = 1.0;
#pragma unroll
    for (int d = 0; d < N; ++d) vol *= g.h[d] / 6.0;
    double sK = 0.0, sM = 0.0;
    for (int i = 0; i < nmodes; ++i) {
        const double *__restrict__ phi = Phi + i * g.nnode * N;
        double ue[NPE][N];
#pragma unroll
        for (int mn = 0; mn < NPE; ++mn) {
            int c[N];
#pragma unroll
            for (int d = 0; d < N; ++d) c[d] = ec[d] + node_bit<N>(mn, d);
            const long long nd = flat_index<N>(g.ne, 1, c);
#pragma unroll
            for (int b = 0; b < N; ++b) ue[mn][b] = phi[N * nd + b];
        }
        // phi_e^T K0 phi_e, one node's rows at a time; rolled as in k_stress_gradient (the rows of K0 are not all in flight at once),
        // so the node's own values come from memory again (a cache hit) instead of a register indexed at run time
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
                qK = fma(phi[N * nd + b], acc, qK);
            }
        }
        // phi_e^T M0 phi_e / vol: [[2, 1], [1, 2]] along every axis, component by component
        double qM = 0.0;
#pragma unroll
        for (int b = 0; b < N; ++b) {
            double t[NPE];
#pragma unroll
            for (int j = 0; j < NPE; ++j) t[j] = ue[j][b];
#pragma unroll
            for (int d = 0; d < N; ++d) {
                double r[NPE];
#pragma unroll
                for (int j = 0; j < NPE; ++j) r[j] = 2.0 * t[j] + t[j ^ (1 << d)];
#pragma unroll
                for (int j = 0; j < NPE; ++j) t[j] = r[j];
            }
#pragma unroll
            for (int j = 0; j < NPE; ++j) qM = fma(ue[j][b], t[j], qM);
        }
        sK = fma(cf.cK[i], qK, sK);
        sM = fma(cf.cM[i], qM * vol, sM);
    }
    out[e] = dE[e] * sK + dm[e] * sM;
}

}  // namespace

void launch_modal_mass_apply(const ModalGrid &g, const double *m, const uint8_t *mask, int ncols, const double *X, double *Y,
                             hipStream_t s) {
    const dim3 grd = cell_grid(g.N, g.ne, 1);
    if (g.N == 3) k_modal_mass_apply<3><<<grd, cell_block(), 0, s>>>(g, m, mask, ncols, X, Y);
    else k_modal_mass_apply<2><<<grd, cell_block(), 0, s>>>(g, m, mask, ncols, X, Y);
    VFEM_HIP(hipGetLastError());
}

void launch_modal_project(long long nnode, int N, const uint8_t *mask, int ncols, double *X, hipStream_t s) {
    if (!mask) return;
    k_modal_project<<<(unsigned) ((nnode + 255) / 256), 256, 0, s>>>(nnode, N, mask, ncols, X);
    VFEM_HIP(hipGetLastError());
}

void launch_block_gram(long long n, int ka, const double *A, int kb, const double *B, double *partial, double *G, hipStream_t s) {
    const int k = ka > kb ? ka : kb;
    if (k == 1) gram_tiles<1>(n, ka, A, kb, B, partial, s);
    else if (k <= 4) gram_tiles<4>(n, ka, A, kb, B, partial, s);
    else gram_tiles<GRAM_TILE>(n, ka, A, kb, B, partial, s);
    k_block_gram_finish<<<ka * kb, 256, 0, s>>>(ka * kb, partial, G);
    VFEM_HIP(hipGetLastError());
}

void launch_block_combine(long long n, int kin, int kout, const double *A, const double *C, double *B, hipStream_t s) {
    const long long want = (n + 255) / 256;
    const unsigned blocks = (unsigned) (want < 2048 ? want : 2048);
    for (int j0 = 0; j0 < kout; j0 += COMBINE_TILE) {
        const int jn = kout - j0 < COMBINE_TILE ? kout - j0 : COMBINE_TILE;
        CombineCoef cf;
        for (int r = 0; r < BLOCK_MAX_COLS; ++r)
            for (int j = 0; j < COMBINE_TILE; ++j) cf.c[r][j] = r < kin && j < jn ? C[r * kout + j0 + j] : 0.0;
        k_block_combine<<<blocks, 256, 0, s>>>(n, kin, jn, A, cf, B + (long long) j0 * n);
    }
    VFEM_HIP(hipGetLastError());
}

void launch_modal_gradient(const ModalGrid &g, int nmodes, const double *K0, const ModalCoef &c, const double *dE, const double *dm,
                           const double *Phi, double *out, hipStream_t s) {
    const dim3 grd = cell_grid(g.N, g.ne, 0);
    if (g.N == 3) k_modal_gradient<3><<<grd, cell_block(), 0, s>>>(g, nmodes, K0, c, dE, dm, Phi, out);
    else k_modal_gradient<2><<<grd, cell_block(), 0, s>>>(g, nmodes, K0, c, dE, dm, Phi, out);
    VFEM_HIP(hipGetLastError());
}

}  // namespace vfem
