"""Band storage of the direct solve (``vfem_band_spd_*``, ``vfem_*_direct_solve``; layout documented in include/vfem.h): the
band geometry of a simulator's stiffness matrix and the 64 x 64 tile layout, in numpy."""
import numpy as np

TILE = 64
BAND_CAP_BYTES = 8 << 30          # TensorProductSimulator.solve factorises when the band fits in this (directSolver = "auto")


def band_doubles(n, w):
    """doubles of the tile layout of an n x n band of half-bandwidth w: ceil(n / 64) tile rows of ceil(w / 64) + 2 tiles"""
    return -(-n // TILE) * (-(-w // TILE) + 2) * TILE * TILE


def band_geometry(N, p, ne):
    """(n, w, bytes) of TensorProductSimulator<p,..,p> in N dimensions with ne elements per axis: dofs, half-bandwidth in dofs and
    the band storage of its factorisation.  Nodes are numbered with the last axis fastest, so two nodes of one element are at most
    d = sum_a p * stride_a apart and w = N d + N - 1."""
    stride, d = 1, 0
    for a in range(N - 1, -1, -1):
        d += p * stride
        stride *= p * int(ne[a]) + 1
    n, w = N * stride, N * d + N - 1
    return n, w, band_doubles(n, w) * 8


def band_pack(A, w):
    """the lower band (j <= i <= j + w) of the n x n matrix A (dense array or scipy sparse) in the tile layout, flat; padding rows
    carry the identity"""
    n = A.shape[0]
    nb, bt = -(-n // TILE), -(-w // TILE)
    out = np.zeros((nb, bt + 2, TILE, TILE))
    if hasattr(A, "tocoo"):
        C = A.tocoo()
        C.sum_duplicates()
        i, j, v = C.row.astype(np.int64), C.col.astype(np.int64), C.data
        keep = (j <= i) & (i - j <= w)
        i, j, v = i[keep], j[keep], v[keep]
    else:
        A = np.asarray(A, dtype=np.float64)
        i, j = np.tril_indices(n)
        keep = i - j <= w
        i, j = i[keep], j[keep]
        v = A[i, j]
    out[i // TILE, i // TILE - j // TILE, i % TILE, j % TILE] = v
    pad = np.arange(n, nb * TILE)
    out[pad // TILE, 0, pad % TILE, pad % TILE] = 1.0
    return out.reshape(-1)


def band_unpack(band, n, w):
    """dense n x n lower triangle of the band held in the tile layout (slots 0..bt; entries outside the band are dropped)"""
    nb, bt = -(-n // TILE), -(-w // TILE)
    B = np.asarray(band, dtype=np.float64).reshape(nb, bt + 2, TILE, TILE)
    out = np.zeros((nb * TILE, nb * TILE))
    for I in range(nb):
        for d in range(min(bt, I) + 1):
            J = I - d
            out[I * TILE:(I + 1) * TILE, J * TILE:(J + 1) * TILE] = B[I, d]
    out = out[:n, :n]
    return np.tril(out) - np.tril(out, -w - 1)
