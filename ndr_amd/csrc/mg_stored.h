// What the two hierarchies with stored Galerkin stencils (hom_mg.hip: the periodic cells; thermal_mg.hip: scalar conduction) share
// on the host beside the cycle itself (mg_cycle.h): how far a grid is coarsened, the checks of their entry points, and the V-cycle
// from a zero iterate that preconditions their conjugate gradients.
#pragma once
#include "mg_cycle.h"

#include <array>

namespace vfem {

// "AxB" or "AxBxC"
static inline std::string dims_text(int N, const int *n) {
    std::string t = std::to_string(n[0]);
    for (int d = 1; d < N; ++d) t += "x" + std::to_string(n[d]);
    return t;
}

// The extents of every level, finest first: a level is coarsened while every extent is even and at least 4, at most
// max_coarsenings times (< 0: as far as that allows)
static inline std::vector<std::array<int, 3>> coarsening_ladder(int N, const int *finest, int max_coarsenings) {
    std::vector<std::array<int, 3>> levels(1, std::array<int, 3>{finest[0], finest[1], N == 3 ? finest[2] : 1});
    while (max_coarsenings < 0 || (int) levels.size() - 1 < max_coarsenings) {
        std::array<int, 3> n = levels.back();
        bool ok = true;
        for (int d = 0; d < N; ++d) ok = ok && n[d] % 2 == 0 && n[d] >= 4;
        if (!ok) break;
        for (int d = 0; d < N; ++d) n[d] /= 2;
        levels.push_back(n);
    }
    return levels;
}

// "AxBxC, ..." for the refusal of a coarsest level that is too large
static inline std::string ladder_text(int N, const std::vector<std::array<int, 3>> &levels) {
    std::string t;
    for (const std::array<int, 3> &n : levels) t += (t.empty() ? "" : ", ") + dims_text(N, n.data());
    return t;
}

template <class Handle> static void check_level(const Handle *h, int l, const char *who, int last) {
    if (!h) throw Error(std::string(who) + ": null handle");
    if (l < 0 || l > last) throw Error(std::string(who) + ": level " + std::to_string(l) + " out of range");
}

static inline void check_smoothing(int smoothing, const char *who) {
    if (smoothing < 1 || smoothing > 16) throw Error(std::string(who) + ": smoothing must be in [1, 16]");
}

// X = V-cycle(B) from a zero initial guess: `smoothing` ascending sweeps, the coarse correction, `smoothing` descending sweeps.
// Ops{h, B, X, s} is what mg_cycle::vcycle launches; h->vec(0) the doubles of a level-0 vector
template <class Ops, class Handle> static void cycle_from_zero(Handle *h, const double *B, double *X, int smoothing, hipStream_t s) {
    if (h->L() > 0) VFEM_HIP(hipMemsetAsync(X, 0, h->vec(0) * sizeof(double), s));
    Ops o{h, B, X, s};
    mg_cycle::vcycle(o, 0, smoothing, true);
}

}  // namespace vfem
