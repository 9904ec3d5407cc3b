// Load cases of a degree-1 grid: what kernels_loads.hip offers to loads.hip.
//
// Numbering and the node mask are those of modal.h.  A design-dependent load is an element pattern of ke = N 2^N values (dof = N
// node + component, the local node order of K0) times an element multiplier:
//   f = P (f_in + sum_e m[e] Lb + sum_e E[e] Lt),
// Lb the pattern of a body force (vol / 2^N g[a] at every node), Lt that of an eigenstrain (int B^T sigma*).  The patterns depend on
// the voxel and the load only; the caller forms them.
#pragma once
#include "modal.h"

namespace vfem {

constexpr int LOADS_MAX_CASES = 8;
constexpr int LOADS_MAX_KE = 24;        // N 2^N for N = 3

struct LoadPatterns { double Lb[LOADS_MAX_KE], Lt[LOADS_MAX_KE]; };                 // one case: 48 doubles in the kernel arguments
struct LoadCoef { double cK[LOADS_MAX_CASES], cB[LOADS_MAX_CASES], cT[LOADS_MAX_CASES]; };

// f_out = P (f_in + sum_e m[e] Lb + sum_e E[e] Lt): one thread per node gathers its 2^N elements in ascending local-node order.
// m (with Lb) or E (with Lt) may be null, f_in and mask may be null, f_out may be f_in.
void launch_loads_assemble(const ModalGrid &g, const LoadPatterns &p, const double *m, const double *E, const uint8_t *mask,
                           const double *f_in, double *f_out, hipStream_t s);
// g[e] = dE[e] sum_i cK[i] u_ie^T K0 u_ie + dm[e] sum_i cB[i] Lb_i . u_ie + dE[e] sum_i cT[i] Lt_i . u_ie; K0 (ke x ke), Lb and Lt
// ([ncases][ke], either may be null; dm is null with Lb): device
void launch_loads_gradient(const ModalGrid &g, int ncases, const double *K0, const double *Lb, const double *Lt, const LoadCoef &c,
                           const double *dE, const double *dm, const double *U, double *out, hipStream_t s);

}  // namespace vfem
