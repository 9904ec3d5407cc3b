// 64 x 64 fp64 tile pieces shared by the dense SPD inverse (dense_spd.hip) and the band Cholesky (band_spd.hip): the staged tile
// product with a fixed summation order and the diagonal-tile factorisation.  Both translation units inline the same code.
#pragma once
#include "vfem_internal.h"

namespace vfem {

namespace dense {
constexpr int T = 64;        // tile edge
constexpr int S = 65;        // LDS row stride in doubles (odd: column-wise stores are conflict-free)

// s[k][i] <- tile element with global row r and column c (c contiguous in memory); ROWS_ARE_K: the tile's rows are the
// summation index k (s[r][c]), otherwise its columns are (s[c][r])
template <bool ROWS_ARE_K>
__device__ __forceinline__ void stage(double (*s)[S], const double *__restrict__ g, long long ld) {
    const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int r = r0 + 4 * q;
        const double v = g[(long long) r * ld + c];
        if (ROWS_ARE_K) s[r][c] = v;
        else            s[c][r] = v;
    }
}
// acc[x][y] += sum_k sA[k][ti + 16 x] * sB[k][tj + 16 y], k ascending
__device__ __forceinline__ void mac(double acc[4][4], const double (*sA)[S], const double (*sB)[S]) {
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
#pragma unroll 4
    for (int k = 0; k < T; ++k) {
        double a[4], b[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) { a[m] = sA[k][ti + 16 * m]; b[m] = sB[k][tj + 16 * m]; }
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) acc[x][y] = fma(a[x], b[y], acc[x][y]);
    }
}
// acc += opA(A) opB(B) for one pair of 64 x 64 tiles; opA(A)[i][k] = TA ? A[k][i] : A[i][k], opB(B)[k][j] = TB ? B[j][k] : B[k][j]
template <bool TA, bool TB>
__device__ __forceinline__ void tile_product(double acc[4][4], const double *__restrict__ A, const double *__restrict__ B, long long ld,
                                             double (*sA)[S], double (*sB)[S]) {
    __syncthreads();                       // the previous product has been consumed
    stage<TA>(sA, A, ld);
    stage<!TB>(sB, B, ld);
    __syncthreads();
    mac(acc, sA, sB);
}
__device__ __forceinline__ void zero_acc(double acc[4][4]) {
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[x][y] = 0.0;
}
// C[ti + 16 x][tj + 16 y] = sign * acc (+ C when ACCUM)
template <bool ACCUM>
__device__ __forceinline__ void store_acc(const double acc[4][4], double *__restrict__ C, long long ld, double sign) {
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            double *p = C + (long long) (ti + 16 * x) * ld + tj + 16 * y;
            *p = ACCUM ? *p + sign * acc[x][y] : sign * acc[x][y];
        }
}
}  // namespace dense

// Diagonal tile: L_kk (written back, strict upper part zeroed) and D = L_kk^-1 (64 x 64, row-major), both by right-looking elimination.
// The tile and the inverse under construction live in REGISTERS (thread (r0, c) of CD_RG x 64 owns the rows r0 + CD_RG q of column
// c); a step publishes only column j of A and row j of X through LDS (double-buffered: one workgroup barrier per step)
// and every thread scales them itself (the same products a[r][j] * inv, x[j][c] * inv as an in-place scaling, so the result does not
// depend on the thread layout).  With both matrices in LDS and three barriers per step the tile took 97 us (a chain of dependent
// LDS round trips per row of the trailing update), as one wave without workgroup barriers 259 us; a 2187-dof coarsest level has 35
// such tiles in sequence.  info (0 on entry) receives 1 + pivot_base + the tile index of the first non-positive pivot.
#ifndef VFEM_CD_THREADS
#define VFEM_CD_THREADS 1024
#endif
constexpr int CD_THREADS = VFEM_CD_THREADS;                    // 16 waves: the 64 steps of a tile are one chain of latencies, four waves per SIMD overlap them
constexpr int CD_RG = CD_THREADS / 64, CD_Q = 64 / CD_RG;      // thread (r0, c) owns rows r0 + CD_RG q, q < CD_Q, of column c
__device__ __forceinline__ void chol_diag_tile(double *__restrict__ tile, long long ld, double *__restrict__ D, long long pivot_base,
                                               int *__restrict__ info) {
    using namespace dense;
    static_assert(T == 64, "one lane per column of the tile");
    __shared__ double col[2][T], row[2][T];
    const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    double a[CD_Q], x[CD_Q];
#pragma unroll
    for (int q = 0; q < CD_Q; ++q) {
        const int r = r0 + CD_RG * q;
        a[q] = tile[(long long) r * ld + c];
        x[q] = r == c ? 1.0 : 0.0;
    }
    for (int j = 0; j < T; ++j) {
        const int buf = j & 1;
        // publish column j of A (pivot included) and row j of X as they stand
        if (c == j) {
#pragma unroll
            for (int q = 0; q < CD_Q; ++q) col[buf][r0 + CD_RG * q] = a[q];
        }
        if (r0 == (j % CD_RG)) {
            double xv = 0.0;
#pragma unroll
            for (int q = 0; q < CD_Q; ++q) xv = (j / CD_RG) == q ? x[q] : xv;
            row[buf][c] = xv;
        }
        __syncthreads();
        const double piv = col[buf][j];
        if (!(piv > 0.0) && threadIdx.x == 0 && *info == 0) *info = (int) (pivot_base + j + 1);      // (also catches NaN)
        // 1 / sqrt(piv) from the hardware estimate and two Newton steps (a short dependent chain: the correctly rounded sqrt and
        // division cost ~60 dependent instructions per step, and the 64 steps of a tile are one chain); deterministic, within an
        // ulp or two of the rounded values
        double inv = __builtin_amdgcn_rsq(piv);
        inv = inv * fma(-0.5 * piv * inv, inv, 1.5);
        inv = inv * fma(-0.5 * piv * inv, inv, 1.5);
        const double ljj = piv * inv;
        const double lcj = col[buf][c] * inv;          // L[c][j] (used where c > j)
        const double xjc = row[buf][c] * inv;          // X[j][c] (used where c <= j)
#pragma unroll
        for (int q = 0; q < CD_Q; ++q) {               // (selects, no lane-dependent branches: the conditions differ from lane to lane)
            if (CD_RG * q + CD_RG - 1 < j) continue;   // all rows of this slot lie above the pivot row: finished (uniform over the workgroup)
            const int r = r0 + CD_RG * q;
            const double lrj = col[buf][r] * inv;      // L[r][j]
            const double an = (c > j && c <= r) ? fma(-lrj, lcj, a[q]) : (c == j ? lrj : a[q]);
            const double xn = c <= j ? fma(-lrj, xjc, x[q]) : x[q];
            a[q] = r > j ? an : ((r == j && c == j) ? ljj : a[q]);
            x[q] = r > j ? xn : ((r == j && c <= j) ? xjc : x[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < CD_Q; ++q) {
        const int r = r0 + CD_RG * q;
        tile[(long long) r * ld + c] = c <= r ? a[q] : 0.0;
        D[(long long) r * T + c] = c <= r ? x[q] : 0.0;
    }
}

}  // namespace vfem
