"""Band geometry and tile layout of the direct solve (ndr_amd/band.py, include/vfem.h) against the oracles' assembled stiffness
matrices; no GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MATERIAL = os.path.join(ROOT, "VoxelFEM", "examples", "materials", "B9Creator.material")


def _max_offset(K):
    C = K.tocoo()
    nz = C.data != 0
    return int(np.abs(C.row[nz].astype(np.int64) - C.col[nz]).max())


@pytest.mark.parametrize("ne", [(5, 3), (4, 7), (1, 1), (3, 2, 5), (2, 3, 1), (1, 1, 1)])
def test_degree1_band_matches_the_oracle_assembly(ne):
    from ndr_amd import band
    from oracle import vfem_oracle as vo
    N = len(ne)
    o = vo.OracleSim(([0.0] * N, [2.0] + [1.0] * (N - 1)), ne)
    o.read_material(MATERIAL)
    o.set_densities(np.random.default_rng(1).uniform(0.1, 1.0, o.num_elems))
    K = o.assemble()
    n, w, _ = band.band_geometry(N, 1, ne)
    assert n == K.shape[0]
    assert w == _max_offset(K)


@pytest.mark.parametrize("N,p,ne", [(2, 1, (5, 3)), (2, 2, (3, 5)), (2, 2, (1, 1)), (3, 1, (3, 2, 5)), (3, 2, (3, 1, 2)),
                                    (3, 2, (1, 1, 1))])
def test_band_matches_the_generic_oracle_assembly(N, p, ne):
    from ndr_amd import band
    from oracle import generic_oracle as go
    o = go.GenericSim(N, p, ([0.0] * N, [2.0] + [1.0] * (N - 1)), ne, 1.0, 0.3)
    o.rho = np.random.default_rng(2).uniform(0.1, 1.0, o.num_elems)
    K = o.assemble()
    n, w, _ = band.band_geometry(N, p, ne)
    assert n == K.shape[0]
    assert w == _max_offset(K)


def test_band_geometry_of_the_shipped_problems():
    """the sizes the direct solve serves: the reference's --mgl 0 runs and the 3-D grids up to the 8 GiB cap"""
    from ndr_amd import band
    assert band.band_geometry(2, 1, (300, 100))[:2] == (60802, 205)
    assert band.band_geometry(2, 1, (250, 125))[:2] == (63252, 255)
    assert band.band_geometry(3, 1, (45, 21, 21))[:2] == (66792, 1523)
    n, w, nbytes = band.band_geometry(3, 1, (64, 32, 32))
    assert (n, w) == (212355, 3371) and nbytes <= band.BAND_CAP_BYTES
    assert band.band_geometry(3, 1, (128, 64, 64))[2] > band.BAND_CAP_BYTES


@pytest.mark.parametrize("n,w", [(1, 0), (63, 1), (64, 63), (65, 64), (130, 65), (200, 199)])
def test_band_pack_unpack_round_trip(n, w):
    import scipy.sparse as sp
    from ndr_amd import band
    rng = np.random.default_rng(n + w)
    A = rng.standard_normal((n, n))
    A = A + A.T
    A[np.abs(np.subtract.outer(np.arange(n), np.arange(n))) > w] = 0.0
    B = band.band_pack(A, w)
    assert B.size == band.band_doubles(n, w)
    assert np.array_equal(band.band_unpack(B, n, w), np.tril(A))
    assert np.array_equal(band.band_pack(sp.csr_matrix(A), w), B)
    bt = -(-w // 64)
    for i, j in ((n - 1, max(0, n - 1 - w)), (n // 2, max(0, n // 2 - w)), (0, 0)):      # the address vfem.h documents
        assert B[((i // 64) * (bt + 2) + i // 64 - j // 64) * 4096 + (i % 64) * 64 + j % 64] == A[i, j]
    nb = -(-n // 64)
    Bt = B.reshape(nb, bt + 2, 64, 64)
    for i in range(n, nb * 64):                                                            # padding rows: identity
        assert Bt[i // 64, 0, i % 64, i % 64] == 1.0
