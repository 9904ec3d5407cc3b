// Periodic homogenisation kernels (hom.h): the batched matrix-free periodic operator, its node-block Jacobi preconditioner, the
// vector updates and two-stage reductions of the batched PCG, the homogenised tensor, its density gradient and that gradient
// contracted with a matrix.
//
// (The device helpers shared with the multigrid kernels are in hom_device.h.)
// Apply: one thread owns one periodic node and gathers.  It does not walk element by element: for each of the 3^N neighbour
// offsets it first sums the N x N coefficient block  sum_e E_e K0[(own local node, .), (neighbour's local node, .)]  over the
// incident elements, then multiplies the block with the neighbour's values of all S columns.  The moduli and the K0 entries
// are therefore read once per thread, every neighbour value once per column, and the per-thread state is one block, a row of
// three neighbours' S x N values and the S x N accumulators.  The K0 entries come from the stencil table of hom.h
// (hom_build_stencil: zero where an element does not reach the offset), a wave-uniform table read by scalar loads.  Wrapped
// neighbours that coincide (2 elements along an axis) simply contribute once per offset.
//
// Reductions: every block reduces its values in a fixed order (wave shuffles, then the waves in order) and writes one partial per
// block; a second kernel sums the partials in a fixed order.  No floating-point atomics: results are bit-identical run to run.
#include "hom_device.h"

namespace vfem {

namespace {

template <int N>
__global__ __launch_bounds__(HOM_T) void k_hom_apply(HomDims<N> g, const double *__restrict__ stencil, const double *__restrict__ E,
                                                     const double *__restrict__ w, double *__restrict__ out,
                                                     double *__restrict__ partial) {
    using T = HomTraits<N>;
    constexpr int S = T::S, NPE = T::NPE;
    const int t = blockIdx.x * HOM_T + threadIdx.x;
    double dot[S];
#pragma unroll
    for (int s = 0; s < S; ++s) dot[s] = 0.0;
    if (t < g.pn) {
        int nb[N][3];
        hom_neighbours<N>(t, g, nb);
        double Ee[NPE];
        hom_incident_moduli<N>(g, nb, E, Ee);
        double acc[S][N];
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int a = 0; a < N; ++a) acc[s][a] = 0.0;
        // the offsets along all axes but the last: a loop the compiler must not unroll.  Unrolled, all 3^N S N neighbour values and
        // the whole table are requested at kernel entry and spilled; this way one row of three neighbours is in flight.
#pragma unroll 1
        for (int outer = 0; outer < T::NOFF / 3; ++outer) {
            int base;
            if constexpr (N == 2) {
                base = (outer == 0 ? nb[0][0] : outer == 1 ? nb[0][1] : nb[0][2]) * g.n[1];
            } else {
                const int o0 = outer / 3, o1 = outer - 3 * o0;
                base = ((o0 == 0 ? nb[0][0] : o0 == 1 ? nb[0][1] : nb[0][2]) * g.n[1] + (o1 == 0 ? nb[1][0] : o1 == 1 ? nb[1][1] : nb[1][2])) * g.n[2];
            }
#pragma unroll
            for (int last = 0; last < 3; ++last) {
                const int idx = base + nb[N - 1][last];
                const double *tab = stencil + ((outer * 3 + last) * NPE) * N * N;
                // the pin column: the neighbour's value counts as zero (a factor on the block: the loads stay unconditional)
                const double unpinned = idx == 0 ? 0.0 : 1.0;
                double B[N][N];
                hom_offset_block<N>(Ee, tab, unpinned, B);
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
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const long long at = ((long long) s * g.pn + t) * N;
#pragma unroll
            for (int a = 0; a < N; ++a) {
                const double own = w[at + a];
                const double v = t == 0 ? own : acc[s][a];          // the pin row: identity
                out[at + a] = v;
                dot[s] += own * v;
            }
        }
    }
    if (partial) block_reduce_store<S>(dot, partial, gridDim.x);
}

template <int N>
__global__ __launch_bounds__(HOM_T) void k_hom_jacobi(HomDims<N> g, const double *__restrict__ K0, const double *__restrict__ E,
                                                      double *__restrict__ Minv) {
    using T = HomTraits<N>;
    constexpr int KE = T::KE;
    const int t = blockIdx.x * HOM_T + threadIdx.x;
    if (t >= g.pn) return;
    int nb[N][3];
    hom_neighbours<N>(t, g, nb);
    double Ee[T::NPE];
    hom_incident_moduli<N>(g, nb, E, Ee);
    double B[N][N];
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) {
            double v = 0.0;
#pragma unroll
            for (int ln = 0; ln < T::NPE; ++ln) v += Ee[ln] * K0[(ln * N + a) * KE + ln * N + b];
            B[a][b] = v;
        }
    double I[N][N];
    hom_invert_block<N>(B, I);
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) Minv[(long long) t * N * N + a * N + b] = t == 0 ? (a == b ? 1.0 : 0.0) : I[a][b];
}

template <int N>
__global__ __launch_bounds__(HOM_T) void k_hom_rhs(HomDims<N> g, const double *__restrict__ L, const double *__restrict__ E,
                                                   double *__restrict__ b) {
    using T = HomTraits<N>;
    constexpr int S = T::S;
    const int t = blockIdx.x * HOM_T + threadIdx.x;
    if (t >= g.pn) return;
    int nb[N][3];
    hom_neighbours<N>(t, g, nb);
    double Ee[T::NPE];
    hom_incident_moduli<N>(g, nb, E, Ee);
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int a = 0; a < N; ++a) {
            double v = 0.0;
#pragma unroll
            for (int ln = 0; ln < T::NPE; ++ln) v += Ee[ln] * L[(ln * N + a) * S + s];
            b[((long long) s * g.pn + t) * N + a] = t == 0 ? 0.0 : -v;
        }
}

__global__ __launch_bounds__(HOM_T) void k_hom_finish_alpha(const double *__restrict__ partial, int nblocks, HomState *st) {
    const int s = blockIdx.x;
    const double pAp = sum_partials(partial + (long long) s * nblocks, nblocks);
    if (threadIdx.x == 0) {
        const bool go = st->active[s] && pAp > 0.0;
        st->alpha[s] = go ? st->rz[s] / pAp : 0.0;
        if (go) st->iters[s] += 1;
    }
}

template <int N>
__global__ __launch_bounds__(HOM_T) void k_hom_update(HomDims<N> g, const double *__restrict__ Minv, const double *__restrict__ pv,
                                                      const double *__restrict__ Ap, double *__restrict__ x, double *__restrict__ r,
                                                      double *__restrict__ z, const HomState *__restrict__ st,
                                                      double *__restrict__ partial) {
    constexpr int S = HomTraits<N>::S;
    const int t = blockIdx.x * HOM_T + threadIdx.x;
    double red[2 * S];
#pragma unroll
    for (int i = 0; i < 2 * S; ++i) red[i] = 0.0;
    if (t < g.pn) {
        double Mi[N][N];
#pragma unroll
        for (int a = 0; a < N; ++a)
#pragma unroll
            for (int b = 0; b < N; ++b) Mi[a][b] = Minv[(long long) t * N * N + a * N + b];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const double alpha = st->alpha[s];
            const long long at = ((long long) s * g.pn + t) * N;
            double rn[N];
#pragma unroll
            for (int a = 0; a < N; ++a) {
                x[at + a] += alpha * pv[at + a];
                rn[a] = r[at + a] - alpha * Ap[at + a];
                r[at + a] = rn[a];
                red[S + s] += rn[a] * rn[a];
            }
#pragma unroll
            for (int a = 0; a < N; ++a) {
                double zv = 0.0;
#pragma unroll
                for (int b = 0; b < N; ++b) zv += Mi[a][b] * rn[b];
                z[at + a] = zv;
                red[s] += rn[a] * zv;
            }
        }
    }
    block_reduce_store<2 * S>(red, partial, gridDim.x);
}

__global__ __launch_bounds__(HOM_T) void k_hom_finish_beta(const double *__restrict__ partial, int nblocks, int S, HomState *st,
                                                           double tol, int init) {
    const int s = blockIdx.x;
    const double rz = sum_partials(partial + (long long) s * nblocks, nblocks);
    const double rr = sum_partials(partial + (long long) (S + s) * nblocks, nblocks);
    if (threadIdx.x == 0) {
        if (init) {
            st->rz[s] = rz;
            st->bb[s] = rr;
            st->rr[s] = rr;
            st->alpha[s] = 0.0;
            st->beta[s] = 0.0;
            st->iters[s] = 0;
            st->active[s] = rr > 0.0 && rz > 0.0;             // a zero right-hand side is solved by w = 0
        } else if (st->active[s]) {
            st->beta[s] = rz / st->rz[s];
            st->rz[s] = rz;
            st->rr[s] = rr;
            if (rr <= tol * tol * st->bb[s] || !(rz > 0.0)) st->active[s] = 0;
        } else {
            st->beta[s] = 0.0;
        }
    }
}

__global__ __launch_bounds__(HOM_T) void k_hom_direction(long long per_column, const double *__restrict__ z, double *__restrict__ pv,
                                                         const HomState *__restrict__ st) {
    const long long i = (long long) blockIdx.x * HOM_T + threadIdx.x;
    if (i >= per_column) return;
    const double beta = st->beta[blockIdx.y];
    const long long at = (long long) blockIdx.y * per_column + i;
    pv[at] = z[at] + beta * pv[at];
}

template <int N>
__global__ __launch_bounds__(HOM_T) void k_hom_tensor(HomDims<N> g, const double *__restrict__ L, const double *__restrict__ D,
                                                      double vol, const double *__restrict__ E, const double *__restrict__ W,
                                                      double *__restrict__ partial) {
    using T = HomTraits<N>;
    constexpr int S = T::S, NPE = T::NPE;
    double acc[S * S];
#pragma unroll
    for (int i = 0; i < S * S; ++i) acc[i] = 0.0;
    for (int e = blockIdx.x * HOM_T + threadIdx.x; e < g.pn; e += gridDim.x * HOM_T) {
        int nb[N][3], nd[NPE];
        hom_neighbours<N>(e, g, nb);
        hom_element_nodes<N>(g, nb, nd);
        const double Ee = E[e];
#pragma unroll
        for (int q = 0; q < S; ++q) {
            double dot[S];
#pragma unroll
            for (int r = 0; r < S; ++r) dot[r] = vol * D[q * S + r];
#pragma unroll
            for (int m = 0; m < NPE; ++m)
#pragma unroll
                for (int b = 0; b < N; ++b) {
                    const double wv = W[((long long) q * g.pn + nd[m]) * N + b];
#pragma unroll
                    for (int r = 0; r < S; ++r) dot[r] += wv * L[(m * N + b) * S + r];
                }
#pragma unroll
            for (int r = 0; r < S; ++r) acc[q * S + r] += Ee * dot[r];
        }
    }
    block_reduce_store<S * S>(acc, partial, gridDim.x);
}

__global__ __launch_bounds__(HOM_T) void k_hom_tensor_finish(const double *__restrict__ partial, int nblocks, double scale,
                                                             double *__restrict__ Eh) {
    const double v = sum_partials(partial + (long long) blockIdx.x * nblocks, nblocks);
    if (threadIdx.x == 0) Eh[blockIdx.x] = v * scale;
}

template <int N>
__global__ __launch_bounds__(HOM_T) void k_hom_gradient(HomDims<N> g, const double *__restrict__ K0, const double *__restrict__ L,
                                                        const double *__restrict__ D, double vol, const double *__restrict__ W,
                                                        const double *__restrict__ dE, double inv_cell, double *__restrict__ G) {
    using T = HomTraits<N>;
    constexpr int S = T::S, NPE = T::NPE, KE = T::KE;
    const int e = blockIdx.x * HOM_T + threadIdx.x;
    if (e >= g.pn) return;
    int nb[N][3], nd[NPE];
    hom_neighbours<N>(e, g, nb);
    hom_element_nodes<N>(g, nb, nd);
    const double scale = (dE ? dE[e] : 1.0) * inv_cell;
    double *Ge = G + (long long) e * S * S;
#pragma unroll 1
    for (int r = 0; r < S; ++r) {
        double wr[KE], y[KE];
#pragma unroll
        for (int m = 0; m < NPE; ++m)
#pragma unroll
            for (int b = 0; b < N; ++b) wr[m * N + b] = W[((long long) r * g.pn + nd[m]) * N + b];
        // y = K0 w_r + L[:, r], and L[:, q] . w_r for every q
#pragma unroll
        for (int i = 0; i < KE; ++i) {
            const double *K = launder_uniform(K0);             // one row of K0 in flight at a time
            double v = L[i * S + r];
#pragma unroll
            for (int j = 0; j < KE; ++j) v += K[i * KE + j] * wr[j];
            y[i] = v;
        }
#pragma unroll 1
        for (int q = 0; q <= r; ++q) {
            double v = vol * D[q * S + r];
#pragma unroll
            for (int m = 0; m < NPE; ++m)
#pragma unroll
                for (int b = 0; b < N; ++b)
                    v += W[((long long) q * g.pn + nd[m]) * N + b] * y[m * N + b] + L[(m * N + b) * S + q] * wr[m * N + b];
            Ge[q * S + r] = v * scale;
            Ge[r * S + q] = v * scale;
        }
    }
}

// The gradient contracted with an S x S matrix without forming the block: gout[e] = sum_{q <= r} wt[q][r] v_qr scale, v_qr the very
// sum k_hom_gradient stores at (q, r) and (r, q), wt[q][r] = C[q][r] + C[r][q] above the diagonal and C[q][q] on it (hom.hip).  The
// same two rolled loops, so the same 2 KE doubles of per-thread state; a pair whose weight is zero (wave-uniform) is skipped.
template <int N>
__global__ __launch_bounds__(HOM_T) void k_hom_gradient_contract(HomDims<N> g, const double *__restrict__ K0, const double *__restrict__ L,
                                                                 const double *__restrict__ D, double vol, const double *__restrict__ W,
                                                                 const double *__restrict__ dE, double inv_cell,
                                                                 const double *__restrict__ wt, double *__restrict__ gout) {
    using T = HomTraits<N>;
    constexpr int S = T::S, NPE = T::NPE, KE = T::KE;
    const int e = blockIdx.x * HOM_T + threadIdx.x;
    if (e >= g.pn) return;
    int nb[N][3], nd[NPE];
    hom_neighbours<N>(e, g, nb);
    hom_element_nodes<N>(g, nb, nd);
    double acc = 0.0;
#pragma unroll 1
    for (int r = 0; r < S; ++r) {
        double wr[KE], y[KE];
#pragma unroll
        for (int m = 0; m < NPE; ++m)
#pragma unroll
            for (int b = 0; b < N; ++b) wr[m * N + b] = W[((long long) r * g.pn + nd[m]) * N + b];
#pragma unroll
        for (int i = 0; i < KE; ++i) {
            const double *K = launder_uniform(K0);             // one row of K0 in flight at a time
            double v = L[i * S + r];
#pragma unroll
            for (int j = 0; j < KE; ++j) v += K[i * KE + j] * wr[j];
            y[i] = v;
        }
#pragma unroll 1
        for (int q = 0; q <= r; ++q) {
            const double c = wt[q * S + r];
            if (c == 0.0) continue;
            double v = vol * D[q * S + r];
#pragma unroll
            for (int m = 0; m < NPE; ++m)
#pragma unroll
                for (int b = 0; b < N; ++b)
                    v += W[((long long) q * g.pn + nd[m]) * N + b] * y[m * N + b] + L[(m * N + b) * S + q] * wr[m * N + b];
            acc += c * v;
        }
    }
    gout[e] = acc * ((dE ? dE[e] : 1.0) * inv_cell);
}

}  // namespace

#define HOM_DISPATCH(p, call2, call3) do { if ((p).N == 2) { call2; } else { call3; } VFEM_HIP(hipGetLastError()); } while (0)

void launch_hom_apply(const HomProblem &p, const double *w, double *out, double *partial, hipStream_t s) {
    const int nb = hom_node_blocks(p);
    HOM_DISPATCH(p, (k_hom_apply<2><<<nb, HOM_T, 0, s>>>(dims_of<2>(p), p.stencil, p.E, w, out, partial)),
                 (k_hom_apply<3><<<nb, HOM_T, 0, s>>>(dims_of<3>(p), p.stencil, p.E, w, out, partial)));
}

void launch_hom_jacobi(const HomProblem &p, double *Minv, hipStream_t s) {
    const int nb = hom_node_blocks(p);
    HOM_DISPATCH(p, (k_hom_jacobi<2><<<nb, HOM_T, 0, s>>>(dims_of<2>(p), p.K0, p.E, Minv)),
                 (k_hom_jacobi<3><<<nb, HOM_T, 0, s>>>(dims_of<3>(p), p.K0, p.E, Minv)));
}

void launch_hom_rhs(const HomProblem &p, double *b, hipStream_t s) {
    const int nb = hom_node_blocks(p);
    HOM_DISPATCH(p, (k_hom_rhs<2><<<nb, HOM_T, 0, s>>>(dims_of<2>(p), p.L, p.E, b)),
                 (k_hom_rhs<3><<<nb, HOM_T, 0, s>>>(dims_of<3>(p), p.L, p.E, b)));
}

void launch_hom_finish_alpha(const HomGrid &g, const double *partial, HomState *st, hipStream_t s) {
    k_hom_finish_alpha<<<g.S, HOM_T, 0, s>>>(partial, hom_node_blocks(g), st);
    VFEM_HIP(hipGetLastError());
}

void launch_hom_update(const HomProblem &p, const double *Minv, const double *pv, const double *Ap, double *x, double *r, double *z,
                       const HomState *st, double *partial, hipStream_t s) {
    const int nb = hom_node_blocks(p);
    HOM_DISPATCH(p, (k_hom_update<2><<<nb, HOM_T, 0, s>>>(dims_of<2>(p), Minv, pv, Ap, x, r, z, st, partial)),
                 (k_hom_update<3><<<nb, HOM_T, 0, s>>>(dims_of<3>(p), Minv, pv, Ap, x, r, z, st, partial)));
}

void launch_hom_finish_beta(const HomGrid &g, const double *partial, HomState *st, double tol, int init, hipStream_t s) {
    k_hom_finish_beta<<<g.S, HOM_T, 0, s>>>(partial, hom_node_blocks(g), g.S, st, tol, init);
    VFEM_HIP(hipGetLastError());
}

void launch_hom_direction(const HomGrid &g, const double *z, double *pv, const HomState *st, hipStream_t s) {
    const long long per_column = (long long) g.pn * g.N;
    const dim3 grid((unsigned) ((per_column + HOM_T - 1) / HOM_T), (unsigned) g.S);
    k_hom_direction<<<grid, HOM_T, 0, s>>>(per_column, z, pv, st);
    VFEM_HIP(hipGetLastError());
}

void launch_hom_tensor(const HomProblem &p, const double *W, double inv_cell, double *partial, double *Eh, hipStream_t s) {
    const int nb = hom_tensor_blocks(p);
    HOM_DISPATCH(p, (k_hom_tensor<2><<<nb, HOM_T, 0, s>>>(dims_of<2>(p), p.L, p.D, p.vol, p.E, W, partial)),
                 (k_hom_tensor<3><<<nb, HOM_T, 0, s>>>(dims_of<3>(p), p.L, p.D, p.vol, p.E, W, partial)));
    k_hom_tensor_finish<<<p.S * p.S, HOM_T, 0, s>>>(partial, nb, inv_cell, Eh);
    VFEM_HIP(hipGetLastError());
}

void launch_hom_gradient(const HomProblem &p, const double *W, const double *dE, double inv_cell, double *G, hipStream_t s) {
    const int nb = hom_node_blocks(p);
    HOM_DISPATCH(p, (k_hom_gradient<2><<<nb, HOM_T, 0, s>>>(dims_of<2>(p), p.K0, p.L, p.D, p.vol, W, dE, inv_cell, G)),
                 (k_hom_gradient<3><<<nb, HOM_T, 0, s>>>(dims_of<3>(p), p.K0, p.L, p.D, p.vol, W, dE, inv_cell, G)));
}

void launch_hom_gradient_contract(const HomProblem &p, const double *W, const double *dE, double inv_cell, const double *wt, double *g,
                                  hipStream_t s) {
    const int nb = hom_node_blocks(p);
    HOM_DISPATCH(p, (k_hom_gradient_contract<2><<<nb, HOM_T, 0, s>>>(dims_of<2>(p), p.K0, p.L, p.D, p.vol, W, dE, inv_cell, wt, g)),
                 (k_hom_gradient_contract<3><<<nb, HOM_T, 0, s>>>(dims_of<3>(p), p.K0, p.L, p.D, p.vol, W, dE, inv_cell, wt, g)));
}

}  // namespace vfem
