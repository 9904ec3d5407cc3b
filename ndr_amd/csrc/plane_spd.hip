// Exact coarsest-level solve by a block tridiagonal Cholesky over the x planes (the reference factorises the coarsest operator
// with CHOLMOD, VoxelFEM/TensorProductSimulator.hh:834-865, and so takes a coarsest level of any size; the dense inverse of
// dense_spd.hip stops at 40 000 dofs and costs n^3 below that).
//
// Nodes are numbered x slowest, so K -- fixed rows and columns replaced by the identity, as the dense path does -- is block
// tridiagonal over the NX node planes: diagonal blocks A_j of m = 3 NY NZ dofs, couplings C_j = K[plane j, plane j-1] with at most
// 9 nodes x 3 components per row.
//
//   rows       R[n][nb][3 r + c], the 27 neighbour blocks of every node with the Dirichlet treatment applied, copied once from the
//              level's stencil (k_plane_rows_from_stencil, kernels_mg.hip): A_j is its middle third, C_j the third of the plane
//              below, C_{j+1}^T acting on plane j the third of the plane above (K is symmetric: nothing is scattered)
//   factor     S_0 = A_0, S_j = A_j - C_j T_{j-1} C_j^T, T_j = S_j^-1 kept dense.  The Schur term is two sparse-dense products of
//              27 gathers per entry, W = T_{j-1} C_j^T and A_j - C_j W; the inverse is dense_spd_inverse at size m (NX sequential
//              steps, each of them dense work that fills the device); the fixed rows and columns of T_j are zeroed afterwards, so
//              x is 0 and b is ignored there
//   solve      forward z_0 = b_0, z_j = b_j - C_j (T_{j-1} z_{j-1}); backward x_last = T_last z_last, x_j = T_j (z_j - C_{j+1}^T x_{j+1}):
//              a GEMV on one plane's block (k_gemv) and a coupling gather per step, 4 NX - 3 launches, stream-ordered
// Fixed summation order throughout, no atomics: the same operator gives the same bits on every run.
#include "vfem_host.h"

namespace vfem {

namespace {
struct PlaneGrid { int NY, NZ; long long m; };

// dof r of a plane -> node (jj, kk) of the plane and component
__device__ __forceinline__ void plane_dof(const PlaneGrid &g, long long r, int &jj, int &kk, int &comp) {
    const long long node = r / 3;
    comp = (int) (r - node * 3);
    jj = (int) (node / g.NZ);
    kk = (int) (node - (long long) jj * g.NZ);
}

// W = T_{j-1} C_j^T:  W[q][c] = sum over the 9 nodes of plane j-1 next to node(c) of T_{j-1}[q][3 node' + cq] C_j[c][3 node' + cq]
// (Rj: the rows of plane j's nodes)
__global__ void __launch_bounds__(256) k_plane_w(PlaneGrid g, const double *__restrict__ Rj, const double *__restrict__ Tprev,
                                                 double *__restrict__ W) {
    const long long gid = (long long) blockIdx.x * 256 + threadIdx.x;
    if (gid >= g.m * g.m) return;
    const long long q = gid / g.m, c = gid - q * g.m;
    int jj, kk, cc;
    plane_dof(g, c, jj, kk, cc);
    const double *rows = Rj + (c / 3) * 243 + 3 * cc, *t = Tprev + q * g.m;
    double acc = 0.0;
#pragma unroll
    for (int nb = 0; nb < 9; ++nb) {
        const int j2 = jj + nb / 3 - 1, k2 = kk + nb % 3 - 1;
        if (j2 < 0 || j2 >= g.NY || k2 < 0 || k2 >= g.NZ) continue;
        const long long p = 3 * ((long long) j2 * g.NZ + k2);
#pragma unroll
        for (int cq = 0; cq < 3; ++cq) acc = fma(t[p + cq], rows[nb * 9 + cq], acc);
    }
    W[gid] = acc;
}

// S_j = A_j - C_j W (FIRST: S_0 = A_0), written where T_j will stand
template <bool FIRST>
__global__ void __launch_bounds__(256) k_plane_schur(PlaneGrid g, const double *__restrict__ Rj, const double *__restrict__ W,
                                                     double *__restrict__ Sj) {
    const long long gid = (long long) blockIdx.x * 256 + threadIdx.x;
    if (gid >= g.m * g.m) return;
    const long long r = gid / g.m, c = gid - r * g.m;
    int jr, kr, rr, jc, kc, cc;
    plane_dof(g, r, jr, kr, rr);
    plane_dof(g, c, jc, kc, cc);
    const double *rows = Rj + (r / 3) * 243 + 3 * rr;
    const int dj = jc - jr, dk = kc - kr;
    double v = (dj >= -1 && dj <= 1 && dk >= -1 && dk <= 1) ? rows[(9 + (dj + 1) * 3 + dk + 1) * 9 + cc] : 0.0;
    if (!FIRST) {
        double acc = 0.0;
#pragma unroll
        for (int nb = 0; nb < 9; ++nb) {
            const int j2 = jr + nb / 3 - 1, k2 = kr + nb % 3 - 1;
            if (j2 < 0 || j2 >= g.NY || k2 < 0 || k2 >= g.NZ) continue;
            const long long p = 3 * ((long long) j2 * g.NZ + k2);
#pragma unroll
            for (int cq = 0; cq < 3; ++cq) acc = fma(rows[nb * 9 + cq], W[(p + cq) * g.m + c], acc);
        }
        v -= acc;
    }
    Sj[gid] = v;
}

// out = in - C v over one plane: the third of the rows that couples to the plane below (UP = false: C_j, v on plane j-1) or above
// (UP = true: C_{j+1}^T, v on plane j+1).  in and out may be the same vector (every thread reads and writes its own entry)
template <bool UP>
__global__ void __launch_bounds__(256) k_plane_couple(PlaneGrid g, const double *__restrict__ Rj, const double *__restrict__ v,
                                                      const double *in, double *out) {
    const long long r = (long long) blockIdx.x * 256 + threadIdx.x;
    if (r >= g.m) return;
    int jj, kk, rr;
    plane_dof(g, r, jj, kk, rr);
    const double *rows = Rj + (r / 3) * 243 + (UP ? 18 * 9 : 0) + 3 * rr;
    double acc = 0.0;
#pragma unroll
    for (int nb = 0; nb < 9; ++nb) {
        const int j2 = jj + nb / 3 - 1, k2 = kk + nb % 3 - 1;
        if (j2 < 0 || j2 >= g.NY || k2 < 0 || k2 >= g.NZ) continue;
        const long long p = 3 * ((long long) j2 * g.NZ + k2);
#pragma unroll
        for (int cq = 0; cq < 3; ++cq) acc = fma(rows[nb * 9 + cq], v[p + cq], acc);
    }
    out[r] = in[r] - acc;
}

unsigned blocks_for(long long n) { return (unsigned) ((n + 255) / 256); }
}  // namespace

long long plane_spd_bytes_needed(const Dims &d) {
    // (in floating point: a refused grid may have m^2 beyond 2^63)
    const double m = 3.0 * d.NY * d.NZ, Np = (double) ((3LL * d.NY * d.NZ + 63) / 64 * 64);
    const double doubles = (double) d.NX * m * m + 243.0 * (double) d.nn + m * m + 3.0 * (double) d.nn + m   // T, R, W, z, t
                           + 3.0 * Np * Np + Np * 64.0;                                                      // DenseWork L, X, Tm, D
    const double bytes = doubles * sizeof(double);
    return bytes >= 9.0e18 ? (long long) 9.0e18 : (long long) bytes;
}

void plane_spd_factor(PlaneSolver &ps, const Dims &d, const double *S, const uint8_t *mask, DenseWork &w, hipStream_t s) {
    ScopedTimer tm("coarsestPlaneFactorization");
    ps.d = d;
    const long long m = ps.m(), plane_nodes = (long long) d.NY * d.NZ;
    const PlaneGrid g{d.NY, d.NZ, m};
    ps.T.alloc((size_t) d.NX * m * m);
    ps.R.alloc((size_t) d.nn * 243);
    ps.W.reserve((size_t) m * m);
    ps.z.alloc((size_t) d.nn * 3);
    ps.t.alloc((size_t) m);
    launch_plane_rows_from_stencil(d, S, mask, ps.R.p, s);
    for (int j = 0; j < d.NX; ++j) {
        double *Tj = ps.T.p + (size_t) j * m * m;
        const double *Rj = ps.R.p + (size_t) j * plane_nodes * 243;
        if (j == 0) k_plane_schur<true><<<blocks_for(m * m), 256, 0, s>>>(g, Rj, nullptr, Tj);
        else {
            k_plane_w<<<blocks_for(m * m), 256, 0, s>>>(g, Rj, Tj - m * m, ps.W.p);
            k_plane_schur<false><<<blocks_for(m * m), 256, 0, s>>>(g, Rj, ps.W.p, Tj);
        }
        VFEM_HIP(hipGetLastError());
        try { dense_spd_inverse(m, Tj, w, s); }          // synchronises s for its pivot check
        catch (const Error &e) { throw Error(std::string(e.what()) + " in x plane " + std::to_string(j) + " of " + std::to_string(d.NX)); }
        launch_dense_finish_inverse(m, 3, mask + (size_t) j * plane_nodes, Tj, s);
    }
}

void plane_spd_solve(PlaneSolver &ps, const double *b, double *x, hipStream_t s) {
    const Dims &d = ps.d;
    const long long m = ps.m(), plane_nodes = (long long) d.NY * d.NZ;
    const PlaneGrid g{d.NY, d.NZ, m};
    auto T = [&](int j) { return ps.T.p + (size_t) j * m * m; };
    auto R = [&](int j) { return ps.R.p + (size_t) j * plane_nodes * 243; };
    auto z = [&](int j) { return j == 0 ? b : ps.z.p + (size_t) j * m; };      // z_0 = b_0 is read where it stands
    for (int j = 1; j < d.NX; ++j) {
        launch_gemv_sym(m, T(j - 1), z(j - 1), ps.t.p, s);
        k_plane_couple<false><<<blocks_for(m), 256, 0, s>>>(g, R(j), ps.t.p, b + (size_t) j * m, ps.z.p + (size_t) j * m);
    }
    launch_gemv_sym(m, T(d.NX - 1), z(d.NX - 1), x + (size_t) (d.NX - 1) * m, s);
    for (int j = d.NX - 2; j >= 0; --j) {
        k_plane_couple<true><<<blocks_for(m), 256, 0, s>>>(g, R(j), x + (size_t) (j + 1) * m, z(j), ps.z.p + (size_t) j * m);
        launch_gemv_sym(m, T(j), ps.z.p + (size_t) j * m, x + (size_t) j * m, s);
    }
    VFEM_HIP(hipGetLastError());
}

}  // namespace vfem
