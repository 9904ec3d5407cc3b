// The colour order of the multicolour block Gauss-Seidel sweep on a degree-p node grid (smoothingMulticoloredGS, MG.hh:285-340),
// said once for every launcher that walks it (generic.hip, kernels_q2.hip).  Host code only.  A colour is a local node index:
// its nodes have the same position in each of their incident elements, so no two of them share an element.
#pragma once
#include <type_traits>

namespace vfem {

// the nodes of one colour: per axis the first node, the stride and how many.  Kernels take this by value: the layout stays
struct GsColor { int start[3], inc[3], cnt[3]; };

// f(colour) for the colours [first, first + count) of the (p+1)^N in visiting order -- forward: local node index ascending, axis 0
// slowest, so the colours of one x index are consecutive (what a slab driver exchanges halos between); backward: the same order
// reversed.  nn: nodes per axis.  A colour without nodes (a grid of one element has no second boundary node) is skipped; axes
// from N on hold one node.
template <class F>
void for_each_gs_color(int N, int p, const int nn[3], int forward, int first, int count, F &&f) {
    int ncol = 1;
    for (int a = 0; a < N; ++a) ncol *= p + 1;
    for (int i = first; i < first + count && i < ncol; ++i) {
        int m = forward ? i : ncol - 1 - i;                            // MG.hh:293-295
        GsColor col{{0, 0, 0}, {1, 1, 1}, {1, 1, 1}};
        bool empty = false;
        for (int a = N - 1; a >= 0; --a) {
            const int la = m % (p + 1); m /= p + 1;
            col.start[a] = la;
            col.inc[a] = (1 + (la == 0 || la == p ? 1 : 0)) * p;       // MG.hh:301-305: (1 + isBoundary) * degree
            col.cnt[a] = la > nn[a] - 1 ? 0 : (nn[a] - 1 - la) / col.inc[a] + 1;
            empty = empty || col.cnt[a] == 0;
        }
        if (!empty) f(col);
    }
}

// f(X, Y, Z) with the bits 4, 2 and 1 of `bits` as std::integral_constant<int, 0 or 1>: three runtime bits (the node parities of a
// colour) become template arguments of the kernel that f launches
template <class F>
void with_bits3(int bits, F &&f) {
    auto pick = [](bool bit, auto &&g) { if (!bit) g(std::integral_constant<int, 0>{}); else g(std::integral_constant<int, 1>{}); };
    pick(bits & 4, [&](auto x) { pick(bits & 2, [&](auto y) { pick(bits & 1, [&](auto z) { f(x, y, z); }); }); });
}
inline int parity_bits(const GsColor &c) { return 4 * (c.start[0] & 1) + 2 * (c.start[1] & 1) + (c.start[2] & 1); }

}  // namespace vfem
