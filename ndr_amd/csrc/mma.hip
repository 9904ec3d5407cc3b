// The MMA entry points of include/vfem.h (vfem_mma_*).  Handle-free: device pointers and a stream.  Every argument
// is checked before the first device call.  The n-sized work is one kernel pass per evaluation of the dual (kernels_mma.hip); the
// m x m part -- a projected Newton iteration on lambda >= 0 with a backtracking line search -- runs here on the host.
#include "grid_args.h"
#include "mma.h"
#include "vfem_host.h"

#include <algorithm>
#include <cmath>

using namespace vfem;

namespace {

void check_problem(const std::string &w, int64_t n, int m, const double *x, const double *L, const double *U, const double *xmin,
                   const double *xmax, double move, const double *g0, const double *g) {
    if (n < 1) throw Error(w + ": n must be at least 1");
    if (m < 1 || m > MMA_MAX_M) throw Error(w + ": the number of constraints m must be 1 to 8 (got " + std::to_string(m) + ")");
    if (!x || !L || !U || !xmin || !xmax || !g0 || !g) throw Error(w + ": null argument");
    if (!(move > 0.0) || !std::isfinite(move)) throw Error(w + ": move must be positive");
}

// one evaluation of the dual at lambda: the sums of a kernel pass and what the host adds to them
struct DualPoint {
    double lambda[MMA_MAX_M];
    double W;                                   // sum_j psi_j(x_j(lambda)) - lambda . b - 0.5 sum y_i^2
    double grad[MMA_MAX_M];                     // dW/dlambda_i = G_i - b_i - y_i
    double scale[MMA_MAX_M];                    // s_i = G_i + |b_i| + y_i (p, q > 0: the sum of absolute terms is G_i itself)
    double hess[MMA_MAX_M * MMA_MAX_M];         // -d2W/dlambda2 = H + diag(lambda_i > c), m x m row-major
    double residual;                            // max_i |r_i| / s_i, r_i = grad_i where lambda_i > 0, else max(grad_i, 0)
};

struct Dual {
    MmaProblem p;
    const double *b;
    double c;
    hipStream_t s;
    double *work = nullptr;                     // partials, then the finished sums

    // the workspace is stream-ordered, as compliance()'s is (sim.hip): taking and returning it does not synchronise the device
    Dual(const MmaProblem &p_, hipStream_t s_) : p(p_), b(nullptr), c(0.0), s(s_) {
        VFEM_HIP(hipMallocAsync((void **) &work, (size_t) mma_num_acc(p.m) * (MMA_BLOCKS + 1) * sizeof(double), s));
    }
    Dual(const Dual &) = delete;
    Dual &operator=(const Dual &) = delete;
    ~Dual() { if (work) (void) hipFreeAsync(work, s); }
    // Newton needs the sums on the host before it can choose the next lambda: one small copy and one synchronise per pass
    void sums(const double *lambda, int at_x, double *out) {
        const int na = mma_num_acc(p.m);
        double *fin = work + (size_t) na * MMA_BLOCKS;
        launch_mma_dual(p, lambda, at_x, work, fin, s);
        VFEM_HIP(hipMemcpyAsync(out, fin, (size_t) na * sizeof(double), hipMemcpyDeviceToHost, s));
        VFEM_HIP(hipStreamSynchronize(s));
    }
    // b_i = sum_j (p_ij / (U - x) + q_ij / (x - L)) - f_i at the current x
    void constants(const double *f, double *b_out) {
        double out[mma_num_acc(MMA_MAX_M)], zero[MMA_MAX_M] = {0.0};
        sums(zero, 1, out);
        for (int i = 0; i < p.m; ++i) b_out[i] = (double) ((long double) out[1 + i] - (long double) f[i]);
    }
    // what the host adds is summed in extended precision and rounded once
    void eval(const double *lambda, DualPoint &e) {
        const int m = p.m;
        double out[mma_num_acc(MMA_MAX_M)];
        sums(lambda, 0, out);
        long double W = out[0];
        e.residual = 0.0;
        int a = 1 + m;
        for (int i = 0; i < m; ++i) {
            const double y = std::max(0.0, lambda[i] - c);
            e.lambda[i] = lambda[i];
            W -= (long double) lambda[i] * (long double) b[i] + 0.5L * (long double) y * (long double) y;
            e.grad[i] = (double) ((long double) out[1 + i] - (long double) b[i] - (long double) y);
            e.scale[i] = (double) ((long double) out[1 + i] + (long double) std::fabs(b[i]) + (long double) y);
            for (int k = i; k < m; ++k) e.hess[i * m + k] = e.hess[k * m + i] = out[a++];
            if (lambda[i] > c) e.hess[i * m + i] += 1.0;
            const double r = lambda[i] > 0.0 ? std::fabs(e.grad[i]) : std::max(e.grad[i], 0.0);
            e.residual = std::max(e.residual, r / e.scale[i]);
        }
        e.W = (double) W;
        if (!std::isfinite(e.W) || !std::isfinite(e.residual)) throw Error("MMA: the dual function is not finite (are the gradients?)");
    }
};

// (A + delta I) d = r for the symmetric positive semidefinite k x k matrix A, by Cholesky; false: not positive definite
bool solve_spd(int k, const double *A, double delta, const double *r, double *d) {
    double C[MMA_MAX_M * MMA_MAX_M];
    for (int i = 0; i < k; ++i)
        for (int j = 0; j <= i; ++j) {
            double v = A[i * k + j] + (i == j ? delta : 0.0);
            for (int l = 0; l < j; ++l) v -= C[i * k + l] * C[j * k + l];
            if (i == j) {
                if (!(v > 0.0) || !std::isfinite(v)) return false;
                C[i * k + i] = std::sqrt(v);
            } else {
                C[i * k + j] = v / C[j * k + j];
            }
        }
    for (int i = 0; i < k; ++i) {
        double v = r[i];
        for (int l = 0; l < i; ++l) v -= C[i * k + l] * d[l];
        d[i] = v / C[i * k + i];
    }
    for (int i = k - 1; i >= 0; --i) {
        double v = d[i];
        for (int l = i + 1; l < k; ++l) v -= C[l * k + i] * d[l];
        d[i] = v / C[i * k + i];
        if (!std::isfinite(d[i])) return false;
    }
    return true;
}

// max W(lambda) over lambda >= 0.  W is concave and once differentiable; its Hessian jumps where a variable reaches a bound and
// where lambda_i passes c.  Projected Newton: the multipliers at 0 whose gradient points out of the feasible set are held, the
// others take the Newton step of their block (regularised where no variable is strictly inside its bounds), and the step is
// halved until W has risen by the Armijo amount or, near the maximum where a difference of W is rounding noise, until the
// residual has fallen.  Returns the Newton iterations taken; throws at the cap.
int solve_dual(Dual &D, double tol, int max_iter, DualPoint &cur) {
    const int m = D.p.m;
    double lam[MMA_MAX_M] = {0.0};
    D.eval(lam, cur);
    if (cur.residual <= tol) return 0;
    // a first guess of the multipliers' size: the weight of the objective's approximation over that of each violated constraint
    double ref = 0.0;
    {
        const double w0 = cur.W;          // at lambda = 0 this is sum_j psi_j
        for (int i = 0; i < m; ++i) {
            const double G = cur.grad[i] + D.b[i];          // y = 0 here
            lam[i] = cur.grad[i] > 0.0 && G > 0.0 ? std::min(w0 / G, D.c) : 0.0;
            ref = std::max(ref, lam[i]);
        }
        DualPoint guess;
        D.eval(lam, guess);
        if (guess.W > cur.W) cur = guess;
        if (cur.residual <= tol) return 0;
    }
    for (int it = 1; it <= max_iter; ++it) {
        int F[MMA_MAX_M], nf = 0;
        for (int i = 0; i < m; ++i)
            if (cur.lambda[i] > 0.0 || cur.grad[i] > 0.0) F[nf++] = i;
        double A[MMA_MAX_M * MMA_MAX_M], r[MMA_MAX_M], d[MMA_MAX_M], top = 0.0, lmax = ref;
        for (int a = 0; a < nf; ++a) {
            r[a] = cur.grad[F[a]];
            for (int k = 0; k < nf; ++k) A[a * nf + k] = cur.hess[F[a] * m + F[k]];
            top = std::max(top, A[a * nf + a]);
        }
        for (int i = 0; i < m; ++i) lmax = std::max(lmax, cur.lambda[i]);
        double delta = 1e-12 * top;
        if (!(delta > 0.0)) delta = 1e-300;
        while (!solve_spd(nf, A, delta, r, d)) {
            delta *= 100.0;
            if (!std::isfinite(delta)) throw Error("vfem_mma_subproblem: the dual Hessian is not finite");
        }
        // where the dual is (nearly) linear the Newton step is unbounded: no further than ten times the multipliers' size
        double dmax = 0.0;
        for (int a = 0; a < nf; ++a) dmax = std::max(dmax, std::fabs(d[a]));
        const double cap = 10.0 * std::max(lmax, 1e-300);
        if (lmax > 0.0 && dmax > cap)
            for (int a = 0; a < nf; ++a) d[a] *= cap / dmax;
        DualPoint trial;
        bool accepted = false;
        double t = 1.0;
        for (int h = 0; h < 60 && !accepted; ++h, t *= 0.5) {
            double slope = 0.0;
            bool moved = false;
            for (int i = 0; i < m; ++i) lam[i] = cur.lambda[i];
            for (int a = 0; a < nf; ++a) {
                lam[F[a]] = std::max(0.0, cur.lambda[F[a]] + t * d[a]);
                slope += cur.grad[F[a]] * (lam[F[a]] - cur.lambda[F[a]]);
                moved = moved || lam[F[a]] != cur.lambda[F[a]];
            }
            if (!moved) break;
            D.eval(lam, trial);
            accepted = trial.W >= cur.W + 1e-4 * slope || trial.residual <= 0.9 * cur.residual;
        }
        if (!accepted)
            throw Error("vfem_mma_subproblem: the line search of the dual found no better point at iteration " + std::to_string(it) +
                        " (residual " + std::to_string(cur.residual) + " of its scale, tolerance " + std::to_string(tol) + ")");
        cur = trial;
        if (cur.residual <= tol) return it;
    }
    char msg[256];
    snprintf(msg, sizeof msg, "vfem_mma_subproblem: the dual is not solved after %d Newton iterations: residual %.3e of its scale, "
                              "tolerance %.3e", max_iter, cur.residual, tol);
    throw Error(msg);
}

}  // namespace

extern "C" {

int vfem_mma_asymptotes(int64_t n, int iter, const double *x, const double *xold1, const double *xold2, const double *xmin,
                        const double *xmax, double asyinit, double asyincr, double asydecr, double *L, double *U, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_mma_asymptotes";
    if (n < 1) throw Error(w + ": n must be at least 1");
    if (iter < 1) throw Error(w + ": iter counts the steps from 1");
    if (!x || !xmin || !xmax || !L || !U || (iter > 2 && (!xold1 || !xold2))) throw Error(w + ": null argument");
    if (!(asyinit > 0.0) || !std::isfinite(asyinit)) throw Error(w + ": asyinit must be positive");
    if (!(asydecr > 0.0 && asydecr < 1.0)) throw Error(w + ": asydecr must lie in (0, 1)");
    if (!(asyincr >= 1.0) || !std::isfinite(asyincr)) throw Error(w + ": asyincr must be at least 1");
    if (L == U) throw Error(w + ": L and U must be two arrays");
    launch_mma_asymptotes(n, iter, x, xold1, xold2, xmin, xmax, asyinit, asyincr, asydecr, L, U, S(stream));
    VFEM_CATCH
}

int vfem_mma_dual_eval(int64_t n, int m, const double *x, const double *L, const double *U, const double *xmin, const double *xmax,
                       double move, const double *g0, const double *g, const double *b_host, double c, const double *lambda_host,
                       double *W_host, double *grad_host, double *scale_host, double *hess_host, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_mma_dual_eval";
    check_problem(w, n, m, x, L, U, xmin, xmax, move, g0, g);
    if (!b_host || !lambda_host || !W_host || !grad_host || !scale_host || !hess_host) throw Error(w + ": null argument");
    if (!(c >= 0.0)) throw Error(w + ": c must not be negative");
    for (int i = 0; i < m; ++i)
        if (!(lambda_host[i] >= 0.0) || !std::isfinite(lambda_host[i]) || !std::isfinite(b_host[i]))
            throw Error(w + ": lambda must be finite and not negative, b finite");
    Dual D(MmaProblem{n, m, x, L, U, xmin, xmax, g0, g, move}, S(stream));
    D.b = b_host;
    D.c = c;
    DualPoint e;
    D.eval(lambda_host, e);
    *W_host = e.W;
    for (int i = 0; i < m; ++i) {
        grad_host[i] = e.grad[i];
        scale_host[i] = e.scale[i];
        for (int k = 0; k < m; ++k) hess_host[i * m + k] = e.hess[i * m + k];
    }
    VFEM_CATCH
}

int vfem_mma_subproblem(int64_t n, int m, const double *x, const double *L, const double *U, const double *xmin, const double *xmax,
                        double move, const double *f_host, const double *g0, const double *g, double c, double tol, int max_iter,
                        double *xnew, double *lambda_out, double *y_out, int *iters_out, double *residual_out, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_mma_subproblem";
    check_problem(w, n, m, x, L, U, xmin, xmax, move, g0, g);
    if (!f_host || !xnew || !lambda_out) throw Error(w + ": null argument");
    if (!(tol > 0.0) || !std::isfinite(tol)) throw Error(w + ": tol must be positive");
    if (!(c >= 0.0)) throw Error(w + ": c must not be negative");
    if (max_iter < 1) throw Error(w + ": max_iter must be at least 1");
    for (int i = 0; i < m; ++i)
        if (!std::isfinite(f_host[i])) throw Error(w + ": the constraint values must be finite");
    for (const double *in : {x, L, U, xmin, xmax, g0})
        if (overlaps(xnew, n, in, n)) throw Error(w + ": xnew aliases an input");
    if (overlaps(xnew, n, g, (int64_t) m * n)) throw Error(w + ": xnew aliases an input");
    Dual D(MmaProblem{n, m, x, L, U, xmin, xmax, g0, g, move}, S(stream));
    double b[MMA_MAX_M];
    D.constants(f_host, b);
    D.b = b;
    D.c = c;
    DualPoint e;
    const int its = solve_dual(D, tol, max_iter, e);
    launch_mma_primal(D.p, e.lambda, xnew, S(stream));
    for (int i = 0; i < m; ++i) {
        lambda_out[i] = e.lambda[i];
        if (y_out) y_out[i] = std::max(0.0, e.lambda[i] - c);
    }
    if (iters_out) *iters_out = its;
    if (residual_out) *residual_out = e.residual;
    VFEM_HIP(hipStreamSynchronize(S(stream)));
    VFEM_CATCH
}

}  // extern "C"
