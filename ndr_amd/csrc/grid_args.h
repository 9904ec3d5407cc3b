// What the handle-free entry points that take a voxel grid (stress, modal, buckling, loads, thermal, thermal_mg; mma for the
// aliasing check) do with their arguments before the first device call: the grid itself, and the checks every family repeats.
// Host code only.  `w` is the entry point's name, the prefix of every message.
#pragma once
#include "modal.h"

#include <cmath>

namespace vfem {

// do a bytes at a and nb bytes at b share a byte; the same for doubles
static inline bool overlaps_bytes(const void *a, int64_t na, const void *b, int64_t nb) {
    const char *pa = (const char *) a, *pb = (const char *) b;
    return pa < pb + nb && pb < pa + na;
}
static inline bool overlaps(const double *a, int64_t na, const double *b, int64_t nb) {
    return overlaps_bytes(a, na * (int64_t) sizeof(double), b, nb * (int64_t) sizeof(double));
}

// n host values; what: the subject with its verb ("the element matrix is", "the coefficients are")
static inline void check_finite(const std::string &w, const char *what, const double *v, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) throw Error(w + ": " + what + " not finite");
}

// a number of columns, modes or cases
static inline void check_count(const std::string &w, const char *what, int k, int most) {
    if (k < 1 || k > most) throw Error(w + ": " + what + " must be 1 to " + std::to_string(most) + " (got " + std::to_string(k) + ")");
}

// The grid of an entry point: dim first, then the null arguments, then extent, edge length and node count axis by axis.  h may be
// null (edge lengths of 1) unless need_h; others_given is false when another argument that shares the null-argument refusal of
// the grid's (the flattened tensor) is null.
static inline ModalGrid grid_args(const std::string &w, int dim, const int64_t *nelems, const double *h, bool need_h, bool others_given = true) {
    if (dim != 2 && dim != 3) throw Error(w + ": dim must be 2 or 3");
    if (!nelems || (need_h && !h) || !others_given) throw Error(w + ": null argument");
    ModalGrid g;
    g.N = dim;
    g.ne[2] = 1;
    g.h[0] = g.h[1] = g.h[2] = 1.0;
    g.nelem = g.nnode = 1;
    for (int d = 0; d < dim; ++d) {
        if (nelems[d] < 1) throw Error(w + ": every extent must be at least 1 element");
        if (nelems[d] > (1 << 27)) throw Error(w + ": grid too large");
        if (h) {
            if (!(h[d] > 0.0) || !std::isfinite(h[d])) throw Error(w + ": the voxel's edge lengths must be positive");
            g.h[d] = h[d];
        }
        g.ne[d] = (int) nelems[d];
        g.nelem *= nelems[d];
        g.nnode *= nelems[d] + 1;
        if (g.nnode > (1LL << 31)) throw Error(w + ": grid too large (more than 2^31 nodes)");
    }
    return g;
}

// the same with the flattened tensor D of ndr_amd.materials (S x S, S = 3 or 6), which must be there and finite
static inline ModalGrid grid_and_tensor_args(const std::string &w, int dim, const int64_t *nelems, const double *h, const double *D) {
    const ModalGrid g = grid_args(w, dim, nelems, h, true, D != nullptr);
    const int S = dim == 2 ? 3 : 6;
    check_finite(w, "the tensor is", D, S * S);
    return g;
}

// an output `name` of len doubles against the element multipliers and the per-node mask bytes (either may be null), which the
// message calls mult_noun and mask_noun
static inline void check_output(const std::string &w, const char *name, const double *out, int64_t len, const ModalGrid &g,
                                const double *mult, const char *mult_noun, const uint8_t *mask, const char *mask_noun) {
    if (mult && overlaps(out, len, mult, g.nelem)) throw Error(w + ": " + name + " aliases " + mult_noun);
    if (mask && overlaps_bytes(out, len * (int64_t) sizeof(double), mask, g.nnode)) throw Error(w + ": " + name + " aliases " + mask_noun);
}

}  // namespace vfem
