"""CPU: what every handle-free entry point that takes a voxel grid refuses about the grid itself, through one table for one entry
point of each family (stress, natural frequencies, buckling, load cases, heat conduction).  The refusals come before the first
device call, so the device pointers are addresses nobody dereferences and the module runs without a GPU.  The texts, and which
refusal wins where several apply (``dim``, then null arguments, then the axes in order: extent before edge length), are pinned."""
import ctypes

import numpy as np
import pytest

P = ctypes.c_void_p
DEV = [P(0x100000 * (i + 1)) for i in range(8)]         # far apart: no aliasing refusal gets in the way


def _dp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


# the arguments after the grid's, host arrays sized for 3-D (a refused call reads at most the grid's)
_D, _L, _K = np.eye(6), np.ones(24), np.eye(8)
FAMILIES = {
    # name: (takes the edge lengths, arguments after dim, nelems[, h])
    "vfem_stress_fields": (True, lambda: (_dp(_D), DEV[0], DEV[1], DEV[2], DEV[3], DEV[4], None)),
    "vfem_modal_mass_apply": (True, lambda: (DEV[0], DEV[1], 2, DEV[2], DEV[3], None)),
    "vfem_buckling_geom_apply": (True, lambda: (_dp(_D), DEV[0], DEV[1], DEV[2], 2, DEV[3], DEV[4], None)),
    "vfem_loads_assemble": (True, lambda: (_dp(_L), _dp(_L), DEV[0], DEV[1], DEV[2], DEV[3], DEV[4], None)),
    "vfem_thermal_apply": (False, lambda: (_dp(_K), DEV[0], DEV[1], 2, DEV[2], DEV[3], None)),
}

DIM = "dim must be 2 or 3"
NULL = "null argument"
EXTENT = "every extent must be at least 1 element"
LARGE = "grid too large"
NODES = "grid too large (more than 2^31 nodes)"
EDGE = "the voxel's edge lengths must be positive"
GOOD_NE = {2: (7, 5), 3: (6, 4, 5)}
GOOD_H = {2: (0.5, 0.3), 3: (0.5, 0.3, 0.7)}


def _table():
    """(label, dim, nelems or None, h or None, message, the row is about the edge lengths)"""
    rows = []
    for dim in (1, 4):
        rows.append(("dim %d" % dim, dim, GOOD_NE[3], GOOD_H[3], DIM, False))
        rows.append(("dim %d wins over null nelems" % dim, dim, None, GOOD_H[3], DIM, False))
    for N in (2, 3):
        ne, h = GOOD_NE[N], GOOD_H[N]
        rows.append(("%d-D null nelems" % N, N, None, h, NULL, False))
        rows.append(("%d-D null h" % N, N, ne, None, NULL, True))
        rows.append(("%d-D null h wins over an extent of 0" % N, N, (0,) + ne[1:], None, NULL, True))
        for a in range(N):
            at = lambda t, v: t[:a] + (v,) + t[a + 1:]
            rows.append(("%d-D extent 0 on axis %d" % (N, a), N, at(ne, 0), h, EXTENT, False))
            rows.append(("%d-D extent -3 on axis %d" % (N, a), N, at(ne, -3), h, EXTENT, False))
            rows.append(("%d-D extent 2^27 + 1 on axis %d" % (N, a), N, at(ne, 2 ** 27 + 1), h, LARGE, False))
            for v in (0.0, -0.25, np.inf, -np.inf, np.nan):
                rows.append(("%d-D h %r on axis %d" % (N, v, a), N, ne, at(h, v), EDGE, True))
        # the axes in order, and on one axis the extent before the edge length
        rows.append(("%d-D extent 0 on axis 0 wins over h on axis 1" % N, N, (0,) + ne[1:], (h[0], -1.0) + h[2:], EXTENT, False))
        rows.append(("%d-D h on axis 0 wins over extent 0 on axis 1" % N, N, (ne[0], 0) + ne[2:], (np.nan,) + h[1:], EDGE, True))
        rows.append(("%d-D extent 0 wins over h on the same axis" % N, N, ne[:-1] + (0,), h[:-1] + (0.0,), EXTENT, False))
    rows.append(("2-D 2^16 per axis: more than 2^31 nodes", 2, (2 ** 16, 2 ** 16), GOOD_H[2], NODES, False))
    rows.append(("3-D 2^11 per axis: more than 2^31 nodes", 3, (2 ** 11,) * 3, GOOD_H[3], NODES, False))
    rows.append(("3-D 2^27 x 2^4 x 1: the node count passes on axis 1", 3, (2 ** 27, 2 ** 4, 1), GOOD_H[3], NODES, False))
    rows.append(("3-D the node count wins over a later extent of 0", 3, (2 ** 16, 2 ** 16, 0), GOOD_H[3], NODES, False))
    return rows


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_grid_refusals_are_the_same_for_every_family(name):
    from ndr_amd import _lib
    lib = _lib.load()
    takes_h, rest = FAMILIES[name]
    fn = getattr(lib, name)
    seen = 0
    for label, dim, ne, h, message, about_h in _table():
        if about_h and not takes_h:
            continue
        n = None if ne is None else np.asarray(ne, dtype=np.int64)
        e = None if h is None else np.asarray(h, dtype=np.float64)
        head = (dim, _ip(n), _dp(e)) if takes_h else (dim, _ip(n))
        status = fn(*head, *rest())
        text = lib.vfem_last_error().decode()
        assert status == 1, (name, label)
        assert text == name + ": " + message, (name, label, text)
        seen += 1
    assert seen == (60 if takes_h else 29)


def test_a_null_tensor_or_element_matrix_is_refused_where_the_families_put_it():
    """the flattened tensor counts among the grid's null arguments (before the axes); the element matrix of the conduction operator
    comes after the whole grid"""
    from ndr_amd import _lib
    lib = _lib.load()
    n, h = np.array([6, 0, 5], dtype=np.int64), np.array([0.5, 0.3, 0.7])
    for name in ("vfem_stress_fields", "vfem_buckling_geom_apply"):
        args = list(FAMILIES[name][1]())
        args[0] = None
        assert getattr(lib, name)(3, _ip(n), _dp(h), *args) == 1
        assert lib.vfem_last_error().decode() == name + ": " + NULL
        bad = np.eye(6)
        bad[2, 4] = np.inf
        args[0] = _dp(bad)
        assert getattr(lib, name)(3, _ip(n), _dp(h), *args) == 1
        assert lib.vfem_last_error().decode() == name + ": " + EXTENT         # the axes before the tensor's entries
        n[1] = 4
        assert getattr(lib, name)(3, _ip(n), _dp(h), *args) == 1
        assert lib.vfem_last_error().decode() == name + ": the tensor is not finite"
        n[1] = 0
    args = list(FAMILIES["vfem_thermal_apply"][1]())
    args[0] = None
    assert lib.vfem_thermal_apply(3, _ip(n), *args) == 1
    assert lib.vfem_last_error().decode() == "vfem_thermal_apply: " + EXTENT
    n[1] = 4
    assert lib.vfem_thermal_apply(3, _ip(n), *args) == 1
    assert lib.vfem_last_error().decode() == "vfem_thermal_apply: " + NULL
