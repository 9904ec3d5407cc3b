// Kernels of the multigrid preconditioner of the periodic cell problems (hom_mg.h): the Galerkin product of a level's blocks, the
// inverted diagonal blocks, apply / residual / colour sweep over a level's blocks (stored, or level 0's matrix-free ones), the
// periodic transfers, the dense coarsest matrix, the batched product with its inverse and the PCG's unpreconditioned vector step.
//
// Every kernel is a gather in a fixed order: one thread owns what it writes, nothing is accumulated with atomics, so two runs are
// bit-identical.  A level's blocks come from a block source: HomStoredBlocks reads A[offset][i][j][node] (coalesced over the nodes
// of a wave), HomFineBlocks forms sum_e E_e stencil[offset][e] from the moduli of the node's incident elements, the block of
// k_hom_apply (hom_offset_block, hom_device.h).  The loops over the offsets stay rolled: unrolled, every neighbour value of every
// column is requested at once and the kernel spills.
#include "hom_mg.h"

#include "hom_device.h"

namespace vfem {

namespace {

template <int N>
HomDims<N> dims_of(const HomGrid &p) {
    HomDims<N> g;
    for (int d = 0; d < N; ++d) g.n[d] = p.n[d];
    g.pn = p.pn;
    return g;
}

// coordinates of flat node t (last axis fastest)
template <int N>
__device__ __forceinline__ void hom_coords(int t, const HomDims<N> &g, int c[N]) {
#pragma unroll
    for (int d = N - 1; d >= 0; --d) {
        c[d] = t % g.n[d];
        t /= g.n[d];
    }
}

// hom_neighbours from coordinates (each within [0, n_d))
template <int N>
__device__ __forceinline__ void hom_neighbours_at(const int c[N], const HomDims<N> &g, int nb[N][3]) {
#pragma unroll
    for (int d = 0; d < N; ++d) {
        nb[d][0] = c[d] == 0 ? g.n[d] - 1 : c[d] - 1;
        nb[d][1] = c[d];
        nb[d][2] = c[d] + 1 == g.n[d] ? 0 : c[d] + 1;
    }
}

// the blocks of the matrix-free level: the moduli of the node's incident elements and hom_build_stencil's table
template <int N>
struct HomFineBlocks {
    const double *stencil;
    double Ee[1 << N];
    __device__ __forceinline__ void at(const HomBlocks &src, const HomDims<N> &g, const int (&nb)[N][3], int node) {
        stencil = src.A_or_stencil;
        hom_incident_moduli<N>(g, nb, src.E, Ee);
    }
    __device__ __forceinline__ void block(int o, double (&B)[N][N]) const {
        hom_offset_block<N>(Ee, stencil + (o * (1 << N)) * N * N, 1.0, B);
    }
};

// the blocks of a stored level, A[offset][i][j][node]
template <int N>
struct HomStoredBlocks {
    const double *col;
    long long stride;
    __device__ __forceinline__ void at(const HomBlocks &src, const HomDims<N> &g, const int (&nb)[N][3], int node) {
        col = src.A_or_stencil + node;
        stride = g.pn;
    }
    __device__ __forceinline__ void block(int o, double (&B)[N][N]) const {
#pragma unroll
        for (int a = 0; a < N; ++a)
#pragma unroll
            for (int b = 0; b < N; ++b) B[a][b] = col[((o * N + a) * N + b) * stride];
    }
};

// acc[s] += sum over the 3^N neighbour offsets of (block of the offset) w[s][neighbour], the pin's column counting as zero: the
// loop of k_hom_apply over any block source.  The offsets along all axes but the last form a loop the compiler must not unroll.
// (w is not __restrict__: a sweep updates the vector it reads.)
template <int N, class Blocks>
__device__ __forceinline__ void hom_gather(const HomDims<N> &g, const int (&nb)[N][3], const Blocks &src, const double *w,
                                           double (&acc)[HomTraits<N>::S][N]) {
    using T = HomTraits<N>;
    constexpr int S = T::S;
    // the neighbour coordinates as scalars: selected by the rolled loop's counter below, they must not become an indexed array in scratch
    const int x0 = nb[0][0], x1 = nb[0][1], x2 = nb[0][2];
    const int y0 = nb[N - 2][0], y1 = nb[N - 2][1], y2 = nb[N - 2][2];
    const int z[3] = {nb[N - 1][0], nb[N - 1][1], nb[N - 1][2]};
#pragma unroll 1
    for (int outer = 0; outer < T::NOFF / 3; ++outer) {
        int base;
        if constexpr (N == 2) {
            base = (outer == 0 ? x0 : outer == 1 ? x1 : x2) * g.n[1];
        } else {
            const int o0 = outer / 3, o1 = outer - 3 * o0;
            base = ((o0 == 0 ? x0 : o0 == 1 ? x1 : x2) * g.n[1] + (o1 == 0 ? y0 : o1 == 1 ? y1 : y2)) * g.n[2];
        }
#pragma unroll
        for (int last = 0; last < 3; ++last) {
            const int idx = base + z[last];
            const double unpinned = idx == 0 ? 0.0 : 1.0;          // a factor on the block: the loads stay unconditional
            double B[N][N];
            src.block(outer * 3 + last, B);
#pragma unroll
            for (int a = 0; a < N; ++a)
#pragma unroll
                for (int b = 0; b < N; ++b) B[a][b] *= unpinned;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const double *ws = w + ((long long) s * g.pn + idx) * N;
                double wv[N];
#pragma unroll
                for (int b = 0; b < N; ++b) wv[b] = ws[b];
#pragma unroll
                for (int a = 0; a < N; ++a)
#pragma unroll
                    for (int b = 0; b < N; ++b) acc[s][a] += B[a][b] * wv[b];
            }
        }
    }
}

enum { MG_APPLY = 0, MG_RESIDUAL = 1, MG_SWEEP = 2 };

// MG_APPLY: out = A x.  MG_RESIDUAL: out = b - A x.  MG_SWEEP: x += Dinv (b - A x) on the nodes of one colour (out is x).  A is the
// pinned operator: at node 0 the row is the identity.
template <int N, int MODE, class Blocks>
__global__ __launch_bounds__(HOM_T) void k_hom_mg_level(HomDims<N> g, HomBlocks blocks, HomDinv dinv, int colour, const double *x,
                                                        const double *__restrict__ b, double *out) {
    using T = HomTraits<N>;
    constexpr int S = T::S;
    int t = blockIdx.x * HOM_T + threadIdx.x;
    int c[N];
    if constexpr (MODE == MG_SWEEP) {
        // thread -> node of the colour: the half grid n_d / 2, doubled, plus the colour's parity per axis
        if (t >= (g.pn >> N)) return;
#pragma unroll
        for (int d = N - 1; d >= 0; --d) {
            const int half = g.n[d] >> 1;
            c[d] = 2 * (t % half) + axis_bit<N>(colour, d);
            t /= half;
        }
        t = hom_flat<N>(g, c);
    } else {
        if (t >= g.pn) return;
        hom_coords<N>(t, g, c);
    }
    int nb[N][3];
    hom_neighbours_at<N>(c, g, nb);
    Blocks src;
    src.at(blocks, g, nb, t);
    double acc[S][N];
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int a = 0; a < N; ++a) acc[s][a] = 0.0;
    hom_gather<N>(g, nb, src, x, acc);
    double Di[N][N];
    if constexpr (MODE == MG_SWEEP) {
#pragma unroll
        for (int a = 0; a < N; ++a)
#pragma unroll
            for (int bb = 0; bb < N; ++bb) Di[a][bb] = dinv.p[t * dinv.node_stride + (a * N + bb) * dinv.entry_stride];
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const long long at = ((long long) s * g.pn + t) * N;
        double own[N], v[N];
#pragma unroll
        for (int a = 0; a < N; ++a) {
            own[a] = x[at + a];
            const double Ax = t == 0 ? own[a] : acc[s][a];            // the pin row: identity
            v[a] = MODE == MG_APPLY ? Ax : b[at + a] - Ax;
        }
        if constexpr (MODE == MG_SWEEP) {
#pragma unroll
            for (int a = 0; a < N; ++a) {
                double z = 0.0;
#pragma unroll
                for (int bb = 0; bb < N; ++bb) z += Di[a][bb] * v[bb];
                out[at + a] = own[a] + z;
            }
        } else {
#pragma unroll
            for (int a = 0; a < N; ++a) out[at + a] = v[a];
        }
    }
}

// one thread per coarse offset O and coarse node I.  Per axis the fine row node is a = 2 I + da (weight 1 or 1/2), the fine column
// node b = a + of, and b lies in the support of coarse node I + O when db = da + of - 2 O is -1, 0 or +1 (weight 1 or 1/2).  The
// positions are geometric (not wrapped): with two coarse nodes along an axis O = -1 and O = +1 reach the same node and each keeps
// its own terms.
template <int N, class Blocks>
__global__ __launch_bounds__(HOM_T) void k_hom_mg_galerkin(HomDims<N> gf, HomDims<N> gc, HomBlocks blocks, double *__restrict__ Ac) {
    using T = HomTraits<N>;
    constexpr int NOFF = T::NOFF;
    const long long tid = (long long) blockIdx.x * HOM_T + threadIdx.x;
    if (tid >= (long long) NOFF * gc.pn) return;
    const int O = (int) (tid / gc.pn), I = (int) (tid - (long long) O * gc.pn);
    int Ic[N], Od[N];
    hom_coords<N>(I, gc, Ic);
    {
        int v = O;
#pragma unroll
        for (int d = N - 1; d >= 0; --d, v /= 3) Od[d] = v % 3 - 1;
    }
    double acc[N][N];
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) acc[a][b] = 0.0;
#pragma unroll 1
    for (int ia = 0; ia < NOFF; ++ia) {
        int da[N], c[N];
        double wa = 1.0;
        {
            int v = ia;
#pragma unroll
            for (int d = N - 1; d >= 0; --d, v /= 3) {
                da[d] = v % 3 - 1;
                if (da[d] != 0) wa *= 0.5;
                int f = 2 * Ic[d] + da[d];
                c[d] = f < 0 ? f + gf.n[d] : f;                      // 2 I + 1 < n_f always
            }
        }
        int nb[N][3];
        hom_neighbours_at<N>(c, gf, nb);
        Blocks src;
        src.at(blocks, gf, nb, hom_flat<N>(gf, c));
#pragma unroll 1
        for (int io = 0; io < NOFF; ++io) {
            double wb = wa;
            bool reach = true;
            int v = io;
#pragma unroll
            for (int d = N - 1; d >= 0; --d, v /= 3) {
                const int db = da[d] + (v % 3 - 1) - 2 * Od[d];
                if (db < -1 || db > 1) reach = false;
                if (db != 0) wb *= 0.5;
            }
            if (!reach) continue;
            double B[N][N];
            src.block(io, B);
#pragma unroll
            for (int a = 0; a < N; ++a)
#pragma unroll
                for (int b = 0; b < N; ++b) acc[a][b] += wb * B[a][b];
        }
    }
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) Ac[((long long) (O * N + a) * N + b) * gc.pn + I] = acc[a][b];
}

template <int N>
__global__ __launch_bounds__(HOM_T) void k_hom_mg_dinv(HomDims<N> g, const double *__restrict__ A, double *__restrict__ Dinv) {
    const int t = blockIdx.x * HOM_T + threadIdx.x;
    if (t >= g.pn) return;
    constexpr int centre = (HomTraits<N>::NOFF - 1) / 2;            // a level has at least 2 nodes per axis: only offset 0 is the node itself
    double B[N][N], I[N][N];
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) B[a][b] = A[((long long) (centre * N + a) * N + b) * g.pn + t];
    hom_invert_block<N>(B, I);
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) Dinv[(long long) (a * N + b) * g.pn + t] = t == 0 ? (a == b ? 1.0 : 0.0) : I[a][b];
}

// fine nodes 2 J - 1, 2 J, 2 J + 1 per axis with weights 1/2, 1, 1/2
template <int N>
__global__ __launch_bounds__(HOM_T) void k_hom_mg_restrict(HomDims<N> gf, HomDims<N> gc, const double *__restrict__ vf,
                                                           double *__restrict__ vc) {
    using T = HomTraits<N>;
    constexpr int S = T::S;
    const int t = blockIdx.x * HOM_T + threadIdx.x;
    if (t >= gc.pn) return;
    int Jc[N], f[N][3];
    hom_coords<N>(t, gc, Jc);
#pragma unroll
    for (int d = 0; d < N; ++d) {
        f[d][0] = Jc[d] == 0 ? gf.n[d] - 1 : 2 * Jc[d] - 1;
        f[d][1] = 2 * Jc[d];
        f[d][2] = 2 * Jc[d] + 1;
    }
    double acc[S][N];
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int a = 0; a < N; ++a) acc[s][a] = 0.0;
#pragma unroll 1
    for (int o = 0; o < T::NOFF; ++o) {
        int c[N], v = o;
        double wgt = 1.0;
#pragma unroll
        for (int d = N - 1; d >= 0; --d, v /= 3) {
            const int k = v % 3;
            c[d] = k == 0 ? f[d][0] : k == 1 ? f[d][1] : f[d][2];
            if (k != 1) wgt *= 0.5;
        }
        const int idx = hom_flat<N>(gf, c);
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int a = 0; a < N; ++a) acc[s][a] += wgt * vf[((long long) s * gf.pn + idx) * N + a];
    }
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int a = 0; a < N; ++a) vc[((long long) s * gc.pn + t) * N + a] = t == 0 ? 0.0 : acc[s][a];
}

// an even fine index 2 j takes coarse j, an odd one 2 j + 1 coarse j and (j + 1) mod n_c with 1/2 each
template <int N>
__global__ __launch_bounds__(HOM_T) void k_hom_mg_prolong_add(HomDims<N> gf, HomDims<N> gc, const double *__restrict__ vc,
                                                              double *__restrict__ vf) {
    using T = HomTraits<N>;
    constexpr int S = T::S;
    const int t = blockIdx.x * HOM_T + threadIdx.x;
    if (t >= gf.pn) return;
    int fc[N], j[N][2], odd[N];
    hom_coords<N>(t, gf, fc);
#pragma unroll
    for (int d = 0; d < N; ++d) {
        odd[d] = fc[d] & 1;
        j[d][0] = fc[d] >> 1;
        j[d][1] = j[d][0] + 1 == gc.n[d] ? 0 : j[d][0] + 1;
    }
    double acc[S][N];
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int a = 0; a < N; ++a) acc[s][a] = 0.0;
#pragma unroll
    for (int m = 0; m < (1 << N); ++m) {
        int c[N];
        double wgt = 1.0;
        bool used = true;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            const int k = axis_bit<N>(m, d);
            if (k && !odd[d]) used = false;
            if (odd[d]) wgt *= 0.5;
            c[d] = k ? j[d][1] : j[d][0];
        }
        const int idx = hom_flat<N>(gc, c);
        if (!used || idx == 0) continue;                              // the coarse value of the pin counts as zero
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int a = 0; a < N; ++a) acc[s][a] += wgt * vc[((long long) s * gc.pn + idx) * N + a];
    }
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int a = 0; a < N; ++a) vf[((long long) s * gf.pn + t) * N + a] += acc[s][a];
}

// one thread per node writes the node's N rows, offset after offset: coinciding wrapped neighbours add in a fixed order
template <int N, class Blocks>
__global__ __launch_bounds__(HOM_T) void k_hom_mg_dense(HomDims<N> g, HomBlocks blocks, double *__restrict__ M) {
    using T = HomTraits<N>;
    const int t = blockIdx.x * HOM_T + threadIdx.x;
    if (t >= g.pn) return;
    const long long n = (long long) g.pn * N;
    if (t == 0) {
#pragma unroll
        for (int a = 0; a < N; ++a) M[a * n + a] = 1.0;
        return;
    }
    int c[N], nb[N][3];
    hom_coords<N>(t, g, c);
    hom_neighbours_at<N>(c, g, nb);
    Blocks src;
    src.at(blocks, g, nb, t);
#pragma unroll 1
    for (int o = 0; o < T::NOFF; ++o) {
        int cc[N], v = o;
#pragma unroll
        for (int d = N - 1; d >= 0; --d, v /= 3) {
            const int k = v % 3;
            cc[d] = k == 0 ? nb[d][0] : k == 1 ? nb[d][1] : nb[d][2];
        }
        const int idx = hom_flat<N>(g, cc);
        if (idx == 0) continue;
        double B[N][N];
        src.block(o, B);
#pragma unroll
        for (int a = 0; a < N; ++a)
#pragma unroll
            for (int b = 0; b < N; ++b) M[((long long) t * N + a) * n + (long long) idx * N + b] += B[a][b];
    }
}

// y[s] = Ainv x[s] for the S columns: one wave per row, so the dense inverse is read once per V-cycle whatever S is.  Each lane sums
// its columns c = lane, lane + 64, .. in ascending order, then the lanes are summed by shuffles: a fixed order
template <int S>
__global__ __launch_bounds__(HOM_T) void k_hom_mg_gemv(long long n, const double *__restrict__ A, const double *__restrict__ x,
                                                      double *__restrict__ y) {
    const long long row = (long long) blockIdx.x * (HOM_T / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const double *a = A + row * n;
    double acc[S];
#pragma unroll
    for (int s = 0; s < S; ++s) acc[s] = 0.0;
    for (long long c = lane; c < n; c += 64) {
        const double av = a[c];
#pragma unroll
        for (int s = 0; s < S; ++s) acc[s] = fma(av, x[s * n + c], acc[s]);
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
        double r = acc[s];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) r += __shfl_down(r, o, 64);
        if (lane == 0) y[s * n + row] = r;
    }
}

__global__ __launch_bounds__(HOM_T) void k_hom_mg_update(long long per_column, const double *__restrict__ pv, const double *__restrict__ Ap,
                                                         double *__restrict__ x, double *__restrict__ r, const HomState *__restrict__ st) {
    const long long i = (long long) blockIdx.x * HOM_T + threadIdx.x;
    if (i >= per_column) return;
    const double alpha = st->alpha[blockIdx.y];
    const long long at = (long long) blockIdx.y * per_column + i;
    x[at] += alpha * pv[at];
    r[at] -= alpha * Ap[at];
}

template <int N>
__global__ __launch_bounds__(HOM_T) void k_hom_mg_dots(HomDims<N> g, const double *__restrict__ r, const double *__restrict__ z,
                                                       double *__restrict__ partial) {
    constexpr int S = HomTraits<N>::S;
    const int t = blockIdx.x * HOM_T + threadIdx.x;
    double red[2 * S];
#pragma unroll
    for (int i = 0; i < 2 * S; ++i) red[i] = 0.0;
    if (t < g.pn) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const long long at = ((long long) s * g.pn + t) * N;
#pragma unroll
            for (int a = 0; a < N; ++a) {
                const double rv = r[at + a];
                red[s] += rv * z[at + a];
                red[S + s] += rv * rv;
            }
        }
    }
    block_reduce_store<2 * S>(red, partial, gridDim.x);
}

}  // namespace

#define HOM_MG_DISPATCH(g, call2, call3) do { if ((g).N == 2) { call2; } else { call3; } VFEM_HIP(hipGetLastError()); } while (0)

void launch_hom_mg_galerkin(const HomGrid &fine, const HomGrid &coarse, const HomBlocks &src, double *Ac, hipStream_t s) {
    const long long total = (long long) (fine.N == 2 ? 9 : 27) * coarse.pn;
    const unsigned nb = (unsigned) ((total + HOM_T - 1) / HOM_T);
#define ARGS(N) <<<nb, HOM_T, 0, s>>>(dims_of<N>(fine), dims_of<N>(coarse), src, Ac)
    if (src.E) HOM_MG_DISPATCH(fine, (k_hom_mg_galerkin<2, HomFineBlocks<2>> ARGS(2)), (k_hom_mg_galerkin<3, HomFineBlocks<3>> ARGS(3)));
    else HOM_MG_DISPATCH(fine, (k_hom_mg_galerkin<2, HomStoredBlocks<2>> ARGS(2)), (k_hom_mg_galerkin<3, HomStoredBlocks<3>> ARGS(3)));
#undef ARGS
}

void launch_hom_mg_dinv(const HomGrid &g, const double *A, double *Dinv, hipStream_t s) {
    const int nb = hom_node_blocks(g);
    HOM_MG_DISPATCH(g, (k_hom_mg_dinv<2><<<nb, HOM_T, 0, s>>>(dims_of<2>(g), A, Dinv)), (k_hom_mg_dinv<3><<<nb, HOM_T, 0, s>>>(dims_of<3>(g), A, Dinv)));
}

void launch_hom_mg_apply(const HomGrid &g, const double *A, const double *w, double *out, hipStream_t s) {
    const int nb = hom_node_blocks(g);
    const HomBlocks src{A, nullptr};
    const HomDinv none{nullptr, 0, 0};
    HOM_MG_DISPATCH(g, (k_hom_mg_level<2, MG_APPLY, HomStoredBlocks<2>><<<nb, HOM_T, 0, s>>>(dims_of<2>(g), src, none, 0, w, nullptr, out)),
                    (k_hom_mg_level<3, MG_APPLY, HomStoredBlocks<3>><<<nb, HOM_T, 0, s>>>(dims_of<3>(g), src, none, 0, w, nullptr, out)));
}

void launch_hom_mg_residual(const HomGrid &g, const HomBlocks &src, const double *x, const double *b, double *out, hipStream_t s) {
    const int nb = hom_node_blocks(g);
    const HomDinv none{nullptr, 0, 0};
#define ARGS(N) <<<nb, HOM_T, 0, s>>>(dims_of<N>(g), src, none, 0, x, b, out)
    if (src.E) HOM_MG_DISPATCH(g, (k_hom_mg_level<2, MG_RESIDUAL, HomFineBlocks<2>> ARGS(2)), (k_hom_mg_level<3, MG_RESIDUAL, HomFineBlocks<3>> ARGS(3)));
    else HOM_MG_DISPATCH(g, (k_hom_mg_level<2, MG_RESIDUAL, HomStoredBlocks<2>> ARGS(2)), (k_hom_mg_level<3, MG_RESIDUAL, HomStoredBlocks<3>> ARGS(3)));
#undef ARGS
}

void launch_hom_mg_sweep_colour(const HomGrid &g, const HomBlocks &src, const HomDinv &dinv, int colour, double *x, const double *b,
                                hipStream_t s) {
    const int nb = ((g.pn >> g.N) + HOM_T - 1) / HOM_T;
#define ARGS(N) <<<nb, HOM_T, 0, s>>>(dims_of<N>(g), src, dinv, colour, x, b, x)
    if (src.E) HOM_MG_DISPATCH(g, (k_hom_mg_level<2, MG_SWEEP, HomFineBlocks<2>> ARGS(2)), (k_hom_mg_level<3, MG_SWEEP, HomFineBlocks<3>> ARGS(3)));
    else HOM_MG_DISPATCH(g, (k_hom_mg_level<2, MG_SWEEP, HomStoredBlocks<2>> ARGS(2)), (k_hom_mg_level<3, MG_SWEEP, HomStoredBlocks<3>> ARGS(3)));
#undef ARGS
}

void launch_hom_mg_restrict(const HomGrid &fine, const HomGrid &coarse, const double *vf, double *vc, hipStream_t s) {
    const int nb = hom_node_blocks(coarse);
    HOM_MG_DISPATCH(fine, (k_hom_mg_restrict<2><<<nb, HOM_T, 0, s>>>(dims_of<2>(fine), dims_of<2>(coarse), vf, vc)),
                    (k_hom_mg_restrict<3><<<nb, HOM_T, 0, s>>>(dims_of<3>(fine), dims_of<3>(coarse), vf, vc)));
}

void launch_hom_mg_prolong_add(const HomGrid &fine, const HomGrid &coarse, const double *vc, double *vf, hipStream_t s) {
    const int nb = hom_node_blocks(fine);
    HOM_MG_DISPATCH(fine, (k_hom_mg_prolong_add<2><<<nb, HOM_T, 0, s>>>(dims_of<2>(fine), dims_of<2>(coarse), vc, vf)),
                    (k_hom_mg_prolong_add<3><<<nb, HOM_T, 0, s>>>(dims_of<3>(fine), dims_of<3>(coarse), vc, vf)));
}

void launch_hom_mg_dense(const HomGrid &g, const HomBlocks &src, double *M, hipStream_t s) {
    const int nb = hom_node_blocks(g);
#define ARGS(N) <<<nb, HOM_T, 0, s>>>(dims_of<N>(g), src, M)
    if (src.E) HOM_MG_DISPATCH(g, (k_hom_mg_dense<2, HomFineBlocks<2>> ARGS(2)), (k_hom_mg_dense<3, HomFineBlocks<3>> ARGS(3)));
    else HOM_MG_DISPATCH(g, (k_hom_mg_dense<2, HomStoredBlocks<2>> ARGS(2)), (k_hom_mg_dense<3, HomStoredBlocks<3>> ARGS(3)));
#undef ARGS
}

void launch_hom_mg_gemv(const HomGrid &g, const double *Ainv, const double *x, double *y, hipStream_t s) {
    const long long n = (long long) g.pn * g.N;
    const unsigned nb = (unsigned) ((n + HOM_T / 64 - 1) / (HOM_T / 64));
    if (g.S == 3) k_hom_mg_gemv<3><<<nb, HOM_T, 0, s>>>(n, Ainv, x, y);
    else k_hom_mg_gemv<6><<<nb, HOM_T, 0, s>>>(n, Ainv, x, y);
    VFEM_HIP(hipGetLastError());
}

void launch_hom_mg_update(const HomGrid &g, const double *pv, const double *Ap, double *x, double *r, const HomState *st, hipStream_t s) {
    const long long per_column = (long long) g.pn * g.N;
    const dim3 grid((unsigned) ((per_column + HOM_T - 1) / HOM_T), (unsigned) g.S);
    k_hom_mg_update<<<grid, HOM_T, 0, s>>>(per_column, pv, Ap, x, r, st);
    VFEM_HIP(hipGetLastError());
}

void launch_hom_mg_dots(const HomGrid &g, const double *r, const double *z, double *partial, hipStream_t s) {
    const int nb = hom_node_blocks(g);
    HOM_MG_DISPATCH(g, (k_hom_mg_dots<2><<<nb, HOM_T, 0, s>>>(dims_of<2>(g), r, z, partial)), (k_hom_mg_dots<3><<<nb, HOM_T, 0, s>>>(dims_of<3>(g), r, z, partial)));
}

}  // namespace vfem
