// LangelaarFilter (additive-manufacturing overhang filter, TopologyOptimizationFilter.hh:164-278): forward and backward
// marches along the layer axis (the last grid axis, z fastest in memory: flat = (i ny + j) nz + k).
//
// One launch marches H layers of every column.  A workgroup of 1024 threads owns one column per thread over a region of
// RI x RJ columns (32 x 32 on 3-D grids, 1024 x 1 when ny == 1, i.e. 2-D grids passed as {nx, 1, ny}); the inner
// (RI - 2H) x (RJ - 2H) columns are its core, the rest is a halo of width H that is recomputed by the neighbouring
// workgroups.  Every step reads the previous layer's values of the 4 side neighbours from LDS, so an error at the region's
// edge moves inward by one column per step: after H steps the core is still exact (the shrinking trapezoid).  Waves whose
// columns are already outside the valid trapezoid skip the arithmetic.  Each thread reads its column's H values of every input
// array up front (one contiguous run of H doubles per lane) and writes its core results at the end.
#include "vfem_internal.h"

#include <cfloat>

namespace vfem {

namespace {

constexpr int LG_H = 8;          // layers per launch
constexpr int LG_T = 1024;       // threads (= columns) per workgroup

struct PowP {                    // x^p and x^(p-1); p = 40 (the reference's constant) by repeated squaring
    double p;
    bool p40;
    __device__ void operator()(double x, double &xp, double &xp1) const {
        if (p40) {
            const double x2 = x * x, x4 = x2 * x2, x8 = x4 * x4, x16 = x8 * x8, x32 = x16 * x16;
            xp = x32 * x8;
            xp1 = x32 * x4 * x2 * x;
        } else {
            xp = pow(x, p);
            xp1 = pow(x, p - 1.0);
        }
    }
};

__device__ __forceinline__ double smin(double a, double b, double eps, double seps) {
    const double d = a - b;
    return 0.5 * (a + b - sqrt(d * d + eps) + seps);
}
__device__ __forceinline__ double dsmin(double a, double b, double eps, double sign) {   // sign -1: d/da, +1: d/db
    const double d = a - b;
    return 0.5 * (1.0 + sign * d / sqrt(d * d + eps));
}

// a column's values at layers k0 .. k0+H-1 (0 beyond nz); vector loads when `vec` is set: the launcher sets it (runs_aligned16) when nz
// is even and the array starts on a 16-byte boundary, so that every run starts on one
__device__ __forceinline__ void load_run(const double *__restrict__ a, long long base, int k0, int nz, int vec, double v[LG_H]) {
    if (vec) {
#pragma unroll
        for (int t = 0; t < LG_H; t += 2) {
            if (k0 + t < nz) {
                const double2 w = *reinterpret_cast<const double2 *>(a + base + k0 + t);
                v[t] = w.x; v[t + 1] = w.y;
            } else {
                v[t] = 0.0; v[t + 1] = 0.0;
            }
        }
    } else {
#pragma unroll
        for (int t = 0; t < LG_H; ++t) v[t] = k0 + t < nz ? a[base + k0 + t] : 0.0;
    }
}
__device__ __forceinline__ void store_run(double *__restrict__ a, long long base, int k0, int nz, int vec, const double v[LG_H]) {
    if (vec) {
#pragma unroll
        for (int t = 0; t < LG_H; t += 2)
            if (k0 + t < nz) *reinterpret_cast<double2 *>(a + base + k0 + t) = make_double2(v[t], v[t + 1]);
    } else {
#pragma unroll
        for (int t = 0; t < LG_H; ++t)
            if (k0 + t < nz) a[base + k0 + t] = v[t];
    }
}

// region geometry shared by both marches
template <int RJ>
struct Region {
    static constexpr int RI = LG_T / RJ;
    static constexpr int HJ = RJ == 1 ? 0 : LG_H;              // no halo along j when the grid has one column in j
    static constexpr int CI = RI - 2 * LG_H, CJ = RJ - 2 * HJ;   // core
    static constexpr int LW = RJ == 1 ? 1 : RJ + 2;             // LDS row pitch: the region plus a zero ring (none along j in 2-D)
    static constexpr int LN = (RI + 2) * LW;
    int ri, rj, gi, gj, L, ring;
    bool inb, core;
    __device__ Region(int nx, int ny) {
        const int tid = threadIdx.x;
        ri = tid / RJ; rj = tid % RJ;
        gi = (int) blockIdx.x * CI - LG_H + ri;
        gj = (int) blockIdx.y * CJ - HJ + rj;
        inb = gi >= 0 && gi < nx && gj >= 0 && gj < ny;
        core = ri >= LG_H && ri < LG_H + CI && rj >= HJ && rj < HJ + CJ;
        L = (ri + 1) * LW + (RJ == 1 ? 0 : rj + 1);
        ring = min(ri + 1, RI - ri);                            // distance (in i) to the region's edge, one value per row
    }
    // the 4 side neighbours' values plus the element's own one (the support of the element above)
    __device__ __forceinline__ double cross(const double *s) const {
        if (RJ == 1) return s[L] + s[L - LW] + s[L + LW];     // the j neighbours are outside a grid with ny == 1
        return s[L] + s[L - LW] + s[L + LW] + s[L - 1] + s[L + 1];
    }
};

// forward: layers k0 .. k0+H-1.  out / smax of layer k0-1 come from the previous launch.
template <int RJ>
__global__ void __launch_bounds__(LG_T) k_langelaar_fwd(int nx, int ny, int nz, int k0, int vec, double eps, PowP pw, double invq,
                                                        const double *__restrict__ in, double *__restrict__ out,
                                                        double *__restrict__ smax) {
    using R = Region<RJ>;
    __shared__ double sp[2][R::LN];                             // out^p of the previous layer, ping-pong
    const R r(nx, ny);
    for (int e = threadIdx.x; e < 2 * R::LN; e += LG_T) (&sp[0][0])[e] = 0.0;
    __syncthreads();
    const long long base = ((long long) (r.inb ? r.gi : 0) * ny + (r.inb ? r.gj : 0)) * nz;
    double v[LG_H], o[LG_H] = {}, sm[LG_H] = {};
    if (r.inb) {
        load_run(in, base, k0, nz, vec, v);
        if (k0 > 0) { double q1; pw(out[base + k0 - 1], sp[0][r.L], q1); }
    } else {
#pragma unroll
        for (int t = 0; t < LG_H; ++t) v[t] = 0.0;
    }
    __syncthreads();
    const double seps = sqrt(eps);
#pragma unroll
    for (int t = 0; t < LG_H; ++t) {
        const int k = k0 + t;
        if (k >= nz) break;                                     // uniform
        if (r.ring > t + 1) {                                   // inside the valid trapezoid (per row of the region)
            if (k == 0) {
                o[t] = v[t]; sm[t] = 1.0;
            } else {
                const double S = r.cross(sp[t & 1]);
                sm[t] = pow(S, invq);
                o[t] = smin(v[t], sm[t], eps, seps);
            }
            double q1;
            pw(o[t], sp[(t + 1) & 1][r.L], q1);
            if (!r.inb) sp[(t + 1) & 1][r.L] = 0.0;            // outside the grid: not part of any support
        }
        __syncthreads();
    }
    if (r.inb && r.core) {
        store_run(out, base, k0, nz, vec, o);
        store_run(smax, base, k0, nz, vec, sm);
    }
}

// backward: layers k0+H-1 down to k0.  w = lambda dsmin_dx2(vars, smax) S^(1/q-1) of layer k0+H comes from the previous
// launch through w_in (one plane of nx ny values); this launch leaves w of layer k0 in w_out.
template <int RJ>
__global__ void __launch_bounds__(LG_T) k_langelaar_bwd(int nx, int ny, int nz, int k0, int vec, double eps, PowP pw, double pq,
                                                        const double *__restrict__ g, const double *__restrict__ vars,
                                                        const double *__restrict__ outv, const double *__restrict__ smax,
                                                        const double *__restrict__ w_in, double *__restrict__ w_out,
                                                        double *__restrict__ grad) {
    using R = Region<RJ>;
    __shared__ double sp[2][R::LN];                             // out^p of the layer below the current one
    __shared__ double sw[2][R::LN];                             // w of the layer above the current one
    const R r(nx, ny);
    for (int e = threadIdx.x; e < 2 * R::LN; e += LG_T) { (&sp[0][0])[e] = 0.0; (&sw[0][0])[e] = 0.0; }
    __syncthreads();
    const long long base = ((long long) (r.inb ? r.gi : 0) * ny + (r.inb ? r.gj : 0)) * nz;
    const long long plane = (long long) (r.inb ? r.gi : 0) * ny + (r.inb ? r.gj : 0);
    const int top = min(k0 + LG_H, nz) - 1;
    double gv[LG_H], xv[LG_H], ov[LG_H], sv[LG_H], below = 0.0;
    if (r.inb) {
        load_run(g, base, k0, nz, vec, gv);
        load_run(vars, base, k0, nz, vec, xv);
        load_run(outv, base, k0, nz, vec, ov);
        load_run(smax, base, k0, nz, vec, sv);
        if (k0 > 0) below = outv[base + k0 - 1];
        if (top + 1 < nz) sw[0][r.L] = w_in[plane];
    } else {
#pragma unroll
        for (int t = 0; t < LG_H; ++t) { gv[t] = 0.0; xv[t] = 0.0; ov[t] = 0.0; sv[t] = 0.0; }
    }
    double lam[LG_H];
    double wk = 0.0;
    // step s handles layer k = top - s; the register index is t = k - k0 (compile-time after unrolling over t)
#pragma unroll
    for (int t = LG_H - 1; t >= 0; --t) {
        lam[t] = 0.0;
        const int k = k0 + t;
        if (k > top) continue;                                  // uniform: the last chunk is shorter than H
        const int s = top - k;
        // out^p of layer k-1 for the supports of this layer
        double bp = 0.0, q1;
        if (k > 0) pw(t > 0 ? ov[t > 0 ? t - 1 : 0] : below, bp, q1);   // t is a constant after unrolling
        sp[s & 1][r.L] = r.inb ? bp : 0.0;
        __syncthreads();
        if (r.ring > s + 1) {                                   // inside the valid trapezoid (per row of the region)
            double op, op1;
            pw(ov[t], op, op1);
            lam[t] = gv[t] + pq * op1 * r.cross(sw[s & 1]);
            wk = 0.0;
            if (k > 0) {
                const double S = r.cross(sp[s & 1]);
                if (S >= DBL_MIN) wk = lam[t] * dsmin(xv[t], sv[t], eps, 1.0) * (sv[t] / S);   // S^(1/q-1) = smax / S
            }
            sw[(s + 1) & 1][r.L] = r.inb ? wk : 0.0;
        }
    }
    if (r.inb && r.core) {
        double gr[LG_H];
#pragma unroll
        for (int t = 0; t < LG_H; ++t) gr[t] = lam[t] * dsmin(xv[t], sv[t], eps, -1.0);
        store_run(grad, base, k0, nz, vec, gr);
        if (k0 > 0) w_out[plane] = wk;
    }
}

// the 16-byte path of load_run / store_run: an even nz keeps every run of a 16-byte aligned array on the 16-byte grid; an array that
// starts 8 bytes off it (a view into a larger allocation) has every run off it, and the launch takes the scalar path for all arrays
template <class... P>
bool runs_aligned16(int nz, const P *...arrays) {
    return (nz & 1) == 0 && (((reinterpret_cast<uintptr_t>(arrays) & 15u) == 0) && ...);
}

template <int RJ>
void march(int nx, int ny, int nz, double eps, double p, double q, const double *in, double *out, double *smax, hipStream_t s) {
    using R = Region<RJ>;
    const int vec = runs_aligned16(nz, in, out, smax) ? 1 : 0;
    const dim3 grd((nx + R::CI - 1) / R::CI, (ny + R::CJ - 1) / R::CJ);
    const PowP pw{p, p == 40.0};
    for (int k0 = 0; k0 < nz; k0 += LG_H) {
        hipLaunchKernelGGL(k_langelaar_fwd<RJ>, grd, dim3(LG_T), 0, s, nx, ny, nz, k0, vec, eps, pw, 1.0 / q, in, out, smax);
        VFEM_HIP(hipGetLastError());
    }
}

template <int RJ>
void march_back(int nx, int ny, int nz, double eps, double p, double q, const double *g, const double *vars, const double *out,
                const double *smax, double *work, double *grad, hipStream_t s) {
    using R = Region<RJ>;
    const dim3 grd((nx + R::CI - 1) / R::CI, (ny + R::CJ - 1) / R::CJ);
    const PowP pw{p, p == 40.0};
    const long long plane = (long long) nx * ny;
    const int vec = runs_aligned16(nz, g, vars, out, smax, grad) ? 1 : 0;
    int c = 0;
    for (int k0 = ((nz - 1) / LG_H) * LG_H; k0 >= 0; k0 -= LG_H, ++c) {
        const double *w_in = work + (c & 1) * plane;
        double *w_out = work + ((c + 1) & 1) * plane;
        hipLaunchKernelGGL(k_langelaar_bwd<RJ>, grd, dim3(LG_T), 0, s, nx, ny, nz, k0, vec, eps, pw, p / q, g, vars, out, smax,
                           w_in, w_out, grad);
        VFEM_HIP(hipGetLastError());
    }
}

}  // namespace

void launch_langelaar_apply(int nx, int ny, int nz, double eps, double p, double q, const double *in, double *out, double *smax,
                            hipStream_t s) {
    if (ny == 1) march<1>(nx, ny, nz, eps, p, q, in, out, smax, s);
    else march<32>(nx, ny, nz, eps, p, q, in, out, smax, s);
}

void launch_langelaar_backprop(int nx, int ny, int nz, double eps, double p, double q, const double *g, const double *vars,
                               const double *out, const double *smax, double *work, double *grad, hipStream_t s) {
    if (ny == 1) march_back<1>(nx, ny, nz, eps, p, q, g, vars, out, smax, work, grad, s);
    else march_back<32>(nx, ny, nz, eps, p, q, g, vars, out, smax, work, grad, s);
}

}  // namespace vfem
