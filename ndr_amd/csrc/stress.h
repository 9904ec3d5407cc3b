// Element stresses of a degree-1 grid: what kernels_stress.hip offers to stress.hip.
//
// Nodes and elements are numbered with the last axis fastest; u, the adjoint load and lambda are [nodes][N]; element e owns the 2^N
// nodes (e_d + mu_d), its local node index has axis 0 as the most significant bit.  Strain and stress are flattened in the order of
// ndr_amd.materials (xx yy xy / xx yy zz yz xz xy) and hold TENSOR components.
//   eps_e   = sum_j sym(g_j (x) u_j),  g_j[k] = +-(1 / h_k) 2^-(N-1): the element's mean strain (the strain at its centroid)
//   sigma_e = m_e C : eps_e,  vm_e = von Mises (plane stress in 2-D)
#pragma once
#include "vfem_internal.h"

namespace vfem {

// the grid and the material as the kernels take them (by value: a few hundred bytes of kernel arguments, no table on the device)
struct StressProblem {
    int N, S;
    int ne[3];              // elements per axis; ne[2] = 1 in 2-D
    double gs[3];           // 2^-(N-1) / h_k
    double Dm[36];          // S x S row-major: the flattened tensor with its shear columns doubled, so sigma = Dm eps
    long long nelem, nnode;
};

constexpr int STRESS_REDUCE_BLOCKS = 1024;      // partials of the two-stage reductions: a function of nothing, so the order is fixed

// whichever of strain [nelem][S], stress [nelem][S], vm [nelem] is not null
void launch_stress_fields(const StressProblem &p, const double *m, const double *u, double *strain, double *stress, double *vm,
                          hipStream_t s);
// out[0] = J = vmax (sum (vm / vmax)^P)^(1/P) (0 when vmax = 0), out[1] = vmax; partial: STRESS_REDUCE_BLOCKS doubles
void launch_stress_pnorm(long long n, const double *vm, double P, double *partial, double *out, hipStream_t s);
// a[node] = sum over the incident elements, in a fixed order, of (vm_e / J)^(P-1) m_e Bbar_j^T (C : dv_e); 0 where mask (may be
// null; bit c of mask[node] = component c fixed) says so.  work: nelem S doubles of scratch (what each element sends to its nodes)
void launch_stress_adjoint_load(const StressProblem &p, const double *m, const double *u, double J, double P, const uint8_t *mask,
                                double *work, double *a, hipStream_t s);
// g[e] = (vm_e / J)^(P-1) dm[e] vm_e / m_e - dE[e] lambda_e^T K0 u_e; K0: device, ke x ke
void launch_stress_gradient(const StressProblem &p, const double *K0, const double *m, const double *dm, const double *dE,
                            const double *u, const double *lambda, double J, double P, double *g, hipStream_t s);

}  // namespace vfem
