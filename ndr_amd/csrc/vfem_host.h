// Host-only declarations shared by the translation units of the C boundary (capi, sim, mg, mg_slab, design, mlp, coarsest,
// plane_spd, hom, hom_mg, stress, mma, modal, buckling, loads, thermal, thermal_mg and the host half of generic): the try / catch
// frame of an entry point, the section timers, and the few functions that cross files.
#pragma once
#include "vfem_internal.h"

#include <chrono>

// every extern "C" entry point that can fail: error code 1 and vfem_last_error() instead of an exception leaving through a C frame
#define VFEM_TRY try {
#define VFEM_CATCH                                                                              \
    } catch (const std::exception &e) { vfem::set_error(e.what()); return 1; }                  \
      catch (...) { vfem::set_error("unknown error"); return 1; }                               \
    return 0;

static inline hipStream_t S(void *s) { return (hipStream_t) s; }

namespace vfem {

// timer registry (BENCHMARK_* of MeshFEM GlobalBenchmark.hh / Timer.hh): host wall time + call count per named section (the
// registry: capi.hip); sections enclosing only asynchronous launches measure enqueue time unless the caller synchronises (the PCG
// loop of mg_cycle.h does, once per iteration).
void timer_add(const char *name, double seconds);
struct ScopedTimer {
    const char *name;
    std::chrono::steady_clock::time_point t0;
    explicit ScopedTimer(const char *n) : name(n), t0(std::chrono::steady_clock::now()) {}
    ~ScopedTimer() { timer_add(name, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()); }
};

// what launch_dot / launch_sum ask of their scratch: one partial per block (DOT_BLOCKS = 1024, kernels_vec.hip), with room to spare
constexpr size_t REDUCE_SCRATCH_DOUBLES = 2048;
// ComplianceObjective::compliance (TopologyOptimizationObjective.hh:39-41): 0.5 f.u over n dofs, to the host (sim.hip).  The scratch
// is stream-ordered (hipMallocAsync does not synchronise the device): evaluations on different streams share no partial sums.
double compliance(long long n, const double *f, const double *u, hipStream_t s);

// what the set_elasticity_tensor entry points refuse before anything is rebuilt (sim.hip): an n x n flattened tensor that is not
// finite, not symmetric (1e-10 of its largest entry, the bound of the material files) or has a non-positive diagonal entry.
// (Positive definiteness is checked by the host class that parses materials; this is the C boundary's own sanity check.)
void check_flattened_tensor(const double *D, int n);

// Galerkin projection out = Phi^T K Phi of an element matrix (MG.hh:644-648; mg.hip): K, scratch, out are ke x ke with ke = N * npe
// (node-major dofs), Phi(fine node, coarse node) is npe x npe and acts on every component alike.  T = K Phi, then Phi^T T, each
// entry summed over the node index ascending from 0.0.
void galerkin_project(const double *K, int ke, int N, int npe, const double *Phi, double *scratch, double *out);

// MG.hh:57-84 in integer arithmetic (mg.hip): a fine Dirichlet node lying on a coarse element vertex / edge / face constrains all
// coarse nodes of that entity; a fine Dirichlet node strictly inside a coarse element is an error.  Degree-p grids of N axes,
// node index with axis 0 slowest; fine_nn: fine nodes per axis, coarse_ne: coarse elements per axis.
void coarsen_dirichlet_mask(int N, int p, const int fine_nn[3], const std::vector<uint8_t> &fine_mask, const int coarse_ne[3],
                            std::vector<uint8_t> &coarse_mask);

// the trilinear hierarchy's internals that the slab driver (mg_slab.hip) calls; defined in mg.hip
void mg_apply(vfem_mg *mg, int l, const double *u, const double *b, int res, double *out, hipStream_t s);
void mg_smooth(vfem_mg *mg, int l, double *u, const double *b, int forward, hipStream_t s, int first = 0, int count = 8);
// one colour group (half sweep `half` of the sweep order) of level 0 by the marching kernel, result back in u; false: not available
bool mg_smooth_half(vfem_mg *mg, int l, double *u, const double *b, int forward, int half, hipStream_t s, int plane_lo = 0, int plane_hi = -1);
void update_operators(vfem_mg *mg, hipStream_t s);
// one V-cycle (on the iterate x[l]) or one full-multigrid cycle of the residual system b[l] from level l on: what the slab driver
// runs its replicated levels with
void cycle_from_level(vfem_mg *mg, int l, int nsmooth, bool fmg, hipStream_t s);

}  // namespace vfem
