// Direct solve of the stiffness system by a band Cholesky factorisation (the reference's TPS::solve,
// VoxelFEM/TensorProductSimulator.hh:834-865, factorises K with CHOLMOD after removing the Dirichlet rows and columns, and keeps
// the numeric factorisation until the densities change).
//
//   assembly   the lower band of the full-size K from K0, the SIMP moduli and the Dirichlet mask, one thread per stored entry:
//              the sum over the elements incident to both dofs in a fixed order (no atomics).  A fixed dof's row and column are
//              the identity, so the free block factorises exactly as the reference's reduced matrix.
//   factor     blocked right-looking Cholesky on 64 x 64 tiles (dense_tiles.h): per tile row k the diagonal tile with its inverse
//              (one workgroup), the panel L_ik = A_ik L_kk^-T of the tiles below, the update A_ij -= L_ik L_jk^T of the band
//              triangle under it -- three launches per tile row
//   solve      forward and backward substitution, one workgroup marching over the tile rows (one launch per direction and
//              right-hand side); the diagonal blocks are applied as products with the kept L_kk^-1
// Fixed summation order throughout: the same matrix gives the same bits on every run.  Layout: include/vfem.h.
#include "dense_tiles.h"

#include <algorithm>

namespace vfem {

namespace {
constexpr long long TILE = 64 * 64;
__host__ __device__ __forceinline__ long long tile_at(int bt, long long I, long long d) { return (I * (bt + 2) + d) * TILE; }
unsigned blocks_for(long long n) { return (unsigned) std::max<long long>(1, std::min<long long>((n + 255) / 256, 1 << 16)); }
int band_tiles(long long w) { return (int) ((w + 63) / 64); }
}  // namespace

long long band_spd_doubles(long long n, long long w) { return (n + 63) / 64 * (band_tiles(w) + 2) * TILE; }

void band_geometry(int N, int p, const int ne[3], long long &n, long long &w) {
    long long stride = 1, d = 0;
    for (int a = N - 1; a >= 0; --a) {
        d += p * stride;                      // two nodes of one element: at most p planes apart along every axis
        stride *= (long long) p * ne[a] + 1;
    }
    n = N * stride;
    w = N * d + N - 1;
}

// entries the factorisation must not read: above the diagonal or outside the band (zero), padding rows (identity)
__global__ void __launch_bounds__(256) k_band_clean(long long n, long long w, long long nb, int bt, double *__restrict__ band) {
    const long long per_row = (long long) (bt + 1) * TILE;
    for (long long g = (long long) blockIdx.x * 256 + threadIdx.x; g < nb * per_row; g += (long long) gridDim.x * 256) {
        const long long I = g / per_row, d = (g - I * per_row) >> 12;
        const int e = (int) (g & 4095);
        const long long i = I * 64 + (e >> 6), j = (I - d) * 64 + (e & 63);
        double *p = band + tile_at(bt, I, d) + e;
        if (i >= n) *p = i == j ? 1.0 : 0.0;
        else if (j < 0 || j > i || i - j > w) *p = 0.0;
    }
}

struct BandGrid { int ne[3], nn[3]; };

// the stored lower band of K (nb (bt + 1) tiles) from K0 [KE][KE], the moduli E and the Dirichlet mask
template <int N, int P>
__global__ void __launch_bounds__(256) k_band_assemble(long long n, long long w, long long nb, int bt, BandGrid g,
                                                       const double *__restrict__ K0, const double *__restrict__ E,
                                                       const uint8_t *__restrict__ mask, double *__restrict__ band) {
    constexpr int Q1 = P + 1, KE = N * (N == 3 ? Q1 * Q1 * Q1 : Q1 * Q1);
    const long long per_row = (long long) (bt + 1) * TILE;
    for (long long t = (long long) blockIdx.x * 256 + threadIdx.x; t < nb * per_row; t += (long long) gridDim.x * 256) {
        const long long I = t / per_row, d = (t - I * per_row) >> 12;
        const int e = (int) (t & 4095);
        const long long i = I * 64 + (e >> 6), j = (I - d) * 64 + (e & 63);
        double v = 0.0;
        if (i >= n) v = i == j ? 1.0 : 0.0;
        else if (j >= 0 && j <= i && i - j <= w) {
            const long long ni = i / N, nj = j / N;
            const int a = (int) (i - ni * N), b = (int) (j - nj * N);
            if (((mask[ni] >> a) & 1) || ((mask[nj] >> b) & 1)) v = i == j ? 1.0 : 0.0;
            else {
                int xi[3] = {0, 0, 0}, xj[3] = {0, 0, 0}, elo[3] = {0, 0, 0}, ehi[3] = {0, 0, 0};
                long long ri = ni, rj = nj;
                bool shared = true;
#pragma unroll
                for (int ax = N - 1; ax >= 0; --ax) {
                    xi[ax] = (int) (ri % g.nn[ax]); ri /= g.nn[ax];
                    xj[ax] = (int) (rj % g.nn[ax]); rj /= g.nn[ax];
                    const int lo = min(xi[ax], xj[ax]), hi = max(xi[ax], xj[ax]);
                    elo[ax] = hi > P ? (hi - 1) / P : 0;          // first element that reaches node hi (P e + P >= hi)
                    ehi[ax] = min(lo / P, g.ne[ax] - 1);          // last element that starts at or before node lo (P e <= lo)
                    shared = shared && elo[ax] <= ehi[ax];
                }
                if (shared)
                    for (int e0 = elo[0]; e0 <= ehi[0]; ++e0)
                        for (int e1 = elo[1]; e1 <= ehi[1]; ++e1)
                            for (int e2 = elo[2]; e2 <= ehi[2]; ++e2) {
                                const int ee[3] = {e0, e1, e2};
                                long long el = 0;
                                int li = 0, lj = 0;
#pragma unroll
                                for (int ax = 0; ax < N; ++ax) {
                                    el = el * g.ne[ax] + ee[ax];
                                    li = li * Q1 + xi[ax] - P * ee[ax];
                                    lj = lj * Q1 + xj[ax] - P * ee[ax];
                                }
                                v = fma(E[el], K0[(N * li + a) * KE + N * lj + b], v);
                            }
            }
        }
        band[tile_at(bt, I, d) + e] = v;
    }
}

__global__ void __launch_bounds__(CD_THREADS) k_band_chol_diag(int bt, long long k, double *__restrict__ band, int *__restrict__ info) {
    chol_diag_tile(band + tile_at(bt, k, 0), dense::T, band + tile_at(bt, k, bt + 1), k * dense::T, info);
}

// L_ik = A_ik L_kk^-T for the tiles i = k + 1 + blockIdx.x below diagonal tile k
__global__ void __launch_bounds__(256) k_band_chol_panel(int bt, long long k, double *__restrict__ band) {
    using namespace dense;
    __shared__ double sA[T][S], sB[T][S];
    const long long i = k + 1 + blockIdx.x;
    double *Aik = band + tile_at(bt, i, i - k);
    double acc[4][4];
    zero_acc(acc);
    stage<false>(sA, Aik, T);
    stage<false>(sB, band + tile_at(bt, k, bt + 1), T);
    __syncthreads();
    mac(acc, sA, sB);
    __syncthreads();
    store_acc<false>(acc, Aik, T, 1.0);
}

// A_ij -= L_ik L_jk^T over the band triangle below tile row k: blockIdx.x enumerates the pairs k < j <= i
__global__ void __launch_bounds__(256) k_band_chol_update(int bt, long long k, double *__restrict__ band) {
    using namespace dense;
    __shared__ double sA[T][S], sB[T][S];
    const int t = blockIdx.x;
    int a = (int) ((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while (a * (a + 1) / 2 > t) --a;
    while ((a + 1) * (a + 2) / 2 <= t) ++a;
    const long long i = k + 1 + a, j = k + 1 + (t - a * (a + 1) / 2);
    double acc[4][4];
    zero_acc(acc);
    tile_product<false, true>(acc, band + tile_at(bt, i, i - k), band + tile_at(bt, j, j - k), T, sA, sB);
    store_acc<true>(acc, band + tile_at(bt, i, i - j), T, -1.0);
}

constexpr int SV_THREADS = 1024, SV_RG = SV_THREADS / 64, SV_Q = 64 / SV_RG;   // thread (rg, c): column c of the rows rg + SV_RG q

__device__ __forceinline__ double wave_sum(double v) {         // lane 0 holds the sum in a fixed order
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// L y = b in place (x: b in, y out), tile row by tile row: r_k = b_k - sum_d L_{k,k-d} y_{k-d}, y_k = L_kk^-1 r_k
__global__ void __launch_bounds__(SV_THREADS) k_band_forward(long long n, long long nb, int bt, const double *__restrict__ band,
                                                             double *__restrict__ x) {
    __shared__ double r[64];
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    for (long long k = 0; k < nb; ++k) {
        double acc[SV_Q];
#pragma unroll
        for (int q = 0; q < SV_Q; ++q) acc[q] = 0.0;
        const int dmax = (int) (k < bt ? k : bt);
        for (int d = 1; d <= dmax; ++d) {
            const double *L = band + tile_at(bt, k, d);
            const double y = x[(k - d) * 64 + c];                 // tile rows above the last one are complete (< n)
#pragma unroll
            for (int q = 0; q < SV_Q; ++q) acc[q] = fma(L[(rg + SV_RG * q) * 64 + c], y, acc[q]);
        }
#pragma unroll
        for (int q = 0; q < SV_Q; ++q) acc[q] = wave_sum(acc[q]);
        if (c == 0) {
#pragma unroll
            for (int q = 0; q < SV_Q; ++q) {
                const int row = rg + SV_RG * q;
                const long long gi = k * 64 + row;
                r[row] = (gi < n ? x[gi] : 0.0) - acc[q];
            }
        }
        __syncthreads();
        const double *D = band + tile_at(bt, k, bt + 1);
        const double rc = r[c];
#pragma unroll
        for (int q = 0; q < SV_Q; ++q) acc[q] = wave_sum(D[(rg + SV_RG * q) * 64 + c] * rc);
        if (c == 0) {
#pragma unroll
            for (int q = 0; q < SV_Q; ++q) {
                const long long gi = k * 64 + rg + SV_RG * q;
                if (gi < n) x[gi] = acc[q];
            }
        }
        __syncthreads();
    }
}

// L^T x = y in place, tile rows in reverse: v_k = y_k - sum_d L_{k+d,k}^T x_{k+d}, x_k = L_kk^-T v_k
__global__ void __launch_bounds__(SV_THREADS) k_band_backward(long long n, long long nb, int bt, const double *__restrict__ band,
                                                              double *__restrict__ x) {
    __shared__ double part[SV_RG][64], v[64];
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    for (long long k = nb - 1; k >= 0; --k) {
        double acc = 0.0;
        const int dmax = (int) (nb - 1 - k < bt ? nb - 1 - k : bt);
        for (int d = 1; d <= dmax; ++d) {
            const double *L = band + tile_at(bt, k + d, d);
#pragma unroll
            for (int q = 0; q < SV_Q; ++q) {
                const int row = rg + SV_RG * q;
                const long long gi = (k + d) * 64 + row;
                acc = fma(L[row * 64 + c], gi < n ? x[gi] : 0.0, acc);
            }
        }
        part[rg][c] = acc;
        __syncthreads();
        if (threadIdx.x < 64) {
            double s = 0.0;
            for (int g2 = 0; g2 < SV_RG; ++g2) s += part[g2][c];
            const long long gi = k * 64 + c;
            v[c] = (gi < n ? x[gi] : 0.0) - s;
        }
        __syncthreads();
        const double *D = band + tile_at(bt, k, bt + 1);
        acc = 0.0;
#pragma unroll
        for (int q = 0; q < SV_Q; ++q) {
            const int row = rg + SV_RG * q;
            acc = fma(D[row * 64 + c], v[row], acc);
        }
        part[rg][c] = acc;
        __syncthreads();
        if (threadIdx.x < 64) {
            double s = 0.0;
            for (int g2 = 0; g2 < SV_RG; ++g2) s += part[g2][c];
            const long long gi = k * 64 + c;
            if (gi < n) x[gi] = s;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_band_zero_fixed(long long n, int N, const uint8_t *__restrict__ mask, double *__restrict__ x) {
    for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < n; i += (long long) gridDim.x * 256)
        if ((mask[i / N] >> (i % N)) & 1) x[i] = 0.0;
}

void launch_band_clean(long long n, long long w, double *band, hipStream_t s) {
    const long long nb = (n + 63) / 64;
    const int bt = band_tiles(w);
    k_band_clean<<<blocks_for(nb * (bt + 1) * TILE), 256, 0, s>>>(n, w, nb, bt, band);
    VFEM_HIP(hipGetLastError());
}

void band_spd_factor(long long n, long long w, double *band, int *info_dev, hipStream_t s, const char *what) {
    const long long nb = (n + 63) / 64;
    const int bt = band_tiles(w);
    VFEM_HIP(hipMemsetAsync(info_dev, 0, sizeof(int), s));
    for (long long k = 0; k < nb; ++k) {
        k_band_chol_diag<<<1, CD_THREADS, 0, s>>>(bt, k, band, info_dev);
        const int rest = (int) std::min<long long>(bt, nb - 1 - k);
        if (rest > 0) {
            k_band_chol_panel<<<rest, 256, 0, s>>>(bt, k, band);
            k_band_chol_update<<<rest * (rest + 1) / 2, 256, 0, s>>>(bt, k, band);
        }
    }
    VFEM_HIP(hipGetLastError());
    int info = 0;
    VFEM_HIP(hipMemcpyAsync(&info, info_dev, sizeof(int), hipMemcpyDeviceToHost, s));
    VFEM_HIP(hipStreamSynchronize(s));
    if (info != 0)
        throw Error(std::string(what) + " is not positive definite (pivot " + std::to_string(info) + " of " + std::to_string(n) + ")");
}

void band_spd_solve(long long n, long long w, const double *factor, double *x, long long nrhs, hipStream_t s) {
    const long long nb = (n + 63) / 64;
    const int bt = band_tiles(w);
    for (long long r = 0; r < nrhs; ++r) {
        k_band_forward<<<1, SV_THREADS, 0, s>>>(n, nb, bt, factor, x + r * n);
        k_band_backward<<<1, SV_THREADS, 0, s>>>(n, nb, bt, factor, x + r * n);
    }
    VFEM_HIP(hipGetLastError());
}

void band_direct_solve(BandSolver &bs, long long version, int N, int p, const int ne[3], const double *K0, const double *E,
                       const uint8_t *mask, const double *f, double *u, hipStream_t s) {
    long long n, w;
    band_geometry(N, p, ne, n, w);
    if (bs.version != version) {
        bs.version = 0;
        const long long nb = (n + 63) / 64;
        const int bt = band_tiles(w);
        bs.band.alloc((size_t) band_spd_doubles(n, w));
        bs.info.alloc(1);
        BandGrid g{};
        for (int a = 0; a < 3; ++a) { g.ne[a] = a < N ? ne[a] : 1; g.nn[a] = a < N ? p * ne[a] + 1 : 1; }
        const unsigned blocks = blocks_for(nb * (bt + 1) * TILE);
        if (N == 2 && p == 1)      k_band_assemble<2, 1><<<blocks, 256, 0, s>>>(n, w, nb, bt, g, K0, E, mask, bs.band.p);
        else if (N == 2)           k_band_assemble<2, 2><<<blocks, 256, 0, s>>>(n, w, nb, bt, g, K0, E, mask, bs.band.p);
        else if (p == 1)           k_band_assemble<3, 1><<<blocks, 256, 0, s>>>(n, w, nb, bt, g, K0, E, mask, bs.band.p);
        else                       k_band_assemble<3, 2><<<blocks, 256, 0, s>>>(n, w, nb, bt, g, K0, E, mask, bs.band.p);
        VFEM_HIP(hipGetLastError());
        band_spd_factor(n, w, bs.band.p, bs.info.p, s, "stiffness matrix");
        bs.version = version;
        ++bs.factorizations;
    }
    if (u != f) VFEM_HIP(hipMemcpyAsync(u, f, (size_t) n * sizeof(double), hipMemcpyDeviceToDevice, s));
    k_band_zero_fixed<<<blocks_for(n), 256, 0, s>>>(n, N, mask, u);
    VFEM_HIP(hipGetLastError());
    band_spd_solve(n, w, bs.band.p, u, 1, s);
}

}  // namespace vfem
