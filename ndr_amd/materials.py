"""Elasticity tensors and material files (MeshFEM ``ElasticityTensor.hh``, ``Materials.cc``, ``python_bindings/tensors.cc``).

``ElasticityTensor`` is a small host-side value class (numpy only): the flattened ``n x n`` matrix ``D`` of a rank-4 tensor with
minor and major symmetries, n = 3 in 2-D (xx, yy, xy) and n = 6 in 3-D (xx, yy, zz, yz, xz, xy: the order of ``Flattening.hh``).
``D`` holds TENSOR components: a shear row is ``C_yzyz = mu_yz``, with no factor 2, so ``sigma_ij = sum_kl C_ijkl eps_kl`` sums
over both (k, l) and (l, k).  The simulators take such an object through ``ETensor`` / ``readMaterial`` and hand ``D`` to the
library (``vfem_sim_set_elasticity_tensor``); nothing here touches the device.
"""
import json

import numpy as np

__all__ = ["ElasticityTensor", "read_material"]

_FLAT = {2: ((0, 2), (2, 1)), 3: ((0, 5, 4), (5, 1, 3), (4, 3, 2))}          # flattened index of the component pair (i, j)
_PAIRS = {2: ((0, 0), (1, 1), (0, 1)), 3: ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))}
_SYM_TOL = 1e-10                                                              # Materials.cc:174,222,238,263


def _flat_len(dim):
    return 3 if dim == 2 else 6


class ElasticityTensor:
    """``ElasticityTensor(dim=3)`` the symmetric identity (lambda = 0, mu = 1/2); ``ElasticityTensor(E, nu, dim=3)`` isotropic
    (plane stress in 2-D); ``ElasticityTensor(material_file, dim=3)`` any of the material file types."""

    def __init__(self, *args, dim=3):
        if dim not in (2, 3):
            raise RuntimeError("Invalid instance dimension.")
        self._dim = int(dim)
        self._D = np.zeros((_flat_len(dim),) * 2)
        self._iso = None             # (E, nu) while D is what setIsotropic built: the simulators then keep the library's isotropic entry point
        if len(args) == 0:
            self.setIdentity()
        elif len(args) == 1 and isinstance(args[0], ElasticityTensor):
            if args[0]._dim != self._dim:
                raise RuntimeError("Dimension mismatch: %d vs %d" % (args[0]._dim, self._dim))
            self._D, self._iso = args[0]._D.copy(), args[0]._iso
        elif len(args) == 1:
            other = read_material(args[0], self._dim)
            self._D, self._iso = other._D, other._iso
        elif len(args) == 2:
            self.setIsotropic(*args)
        else:
            raise TypeError("ElasticityTensor(), ElasticityTensor(E, nu) or ElasticityTensor(material_file)")

    # ---- access ----
    @property
    def dim(self):
        return self._dim

    @property
    def D(self):
        return self._D.copy()

    @classmethod
    def fromD(cls, D, dim=None):
        """the tensor with flattened matrix ``D`` (3 x 3 or 6 x 6, symmetric to 1e-10 as a material file's)"""
        D = np.array(D, dtype=np.float64)
        if dim is None:
            dim = {3: 2, 6: 3}.get(D.shape[0], 0)
        if dim not in (2, 3) or D.shape != (_flat_len(dim),) * 2:
            raise RuntimeError("Failed to parse material_matrix")
        if np.abs(D - D.T).max() > _SYM_TOL:
            raise RuntimeError("Asymmetric material_matrix")
        t = cls(dim=dim)
        t._D, t._iso = np.triu(D) + np.triu(D, 1).T, None                     # the upper triangle is what is kept (Materials.cc:261-262)
        return t

    def __call__(self, i, j, k, l):
        f = _FLAT[self._dim]
        return float(self._D[f[int(i)][int(j)], f[int(k)][int(l)]])

    def __repr__(self):
        return "ElasticityTensor%dD(\n%s)" % (self._dim, np.array2string(self._D, precision=6, suppress_small=True))

    def __eq__(self, other):
        return isinstance(other, ElasticityTensor) and self._dim == other._dim and np.array_equal(self._D, other._D)

    __hash__ = None

    def fullTensor(self):
        """C[i, j, k, l] as a dim^4 array"""
        n, f = self._dim, np.array(_FLAT[self._dim])
        return self._D[f[:, :, None, None], f[None, None, :, :]].reshape(n, n, n, n)

    def doubleContract(self, eps):
        """sigma = C : eps for a dim x dim matrix (symmetric or not: the minor symmetry of C only sees its symmetric part)"""
        eps = np.asarray(eps, dtype=np.float64).reshape(self._dim, self._dim)
        return np.einsum("ijkl,kl->ij", self.fullTensor(), eps)

    def isPositiveDefinite(self):
        """as an operator on symmetric matrices: D with its shear columns doubled, i.e. the flattened D is itself positive definite"""
        w = np.linalg.eigvalsh(0.5 * (self._D + self._D.T))
        return bool(w.min() > 0.0)

    # ---- setters ----
    def setIdentity(self):
        self._set_lame(0.0, 0.5)
        self._iso = (1.0, 0.0)

    def setIsotropic(self, E, nu):
        E, nu = float(E), float(nu)
        lam = nu * E / (1.0 - nu * nu) if self._dim == 2 else nu * E / ((1.0 + nu) * (1.0 - 2.0 * nu))   # 2-D: plane stress
        self._set_lame(lam, E / (2.0 + 2.0 * nu))
        self._iso = (E, nu)

    def _set_lame(self, lam, mu):
        n, D = self._dim, np.zeros((_flat_len(self._dim),) * 2)
        D[:n, :n] = lam
        D[np.arange(n), np.arange(n)] = lam + 2 * mu
        idx = np.arange(n, D.shape[0])
        D[idx, idx] = mu
        self._D = D

    def setOrthotropic(self, *p):
        """2-D: (Ex, Ey, nuYX, muXY); 3-D: (Ex, Ey, Ez, nuYX, nuZX, nuZY, muYZ, muZX, muXY).  D is the matrix inverse of the
        compliance-like matrix with rows 1/E_i, -nu_ji/E_j and 1/mu on the shear diagonal."""
        p = [float(v) for v in p]
        if len(p) not in (4, 9):
            raise TypeError("setOrthotropic takes 4 (2-D) or 9 (3-D) parameters")
        if len(p) != (4 if self._dim == 2 else 9):
            raise RuntimeError("setOrthotropic3D call on non-3D tensor" if len(p) == 9 else "setOrthotropic2D call on non-2D tensor")
        if self._dim == 2:
            Ex, Ey, nuYX, muXY = p
            S = np.diag([1.0 / Ex, 1.0 / Ey, 1.0 / muXY])
            S[0, 1] = S[1, 0] = -nuYX / Ey
        else:
            Ex, Ey, Ez, nuYX, nuZX, nuZY, muYZ, muZX, muXY = p
            S = np.diag([1.0 / Ex, 1.0 / Ey, 1.0 / Ez, 1.0 / muYZ, 1.0 / muZX, 1.0 / muXY])
            S[0, 1] = S[1, 0] = -nuYX / Ey
            S[0, 2] = S[2, 0] = -nuZX / Ez
            S[1, 2] = S[2, 1] = -nuZY / Ez
        D = np.linalg.inv(S)
        self._D, self._iso = 0.5 * (D + D.T), None

    def getOrthotropicParameters(self):
        """the arguments of ``setOrthotropic`` (assuming the tensor is orthotropic in these axes)"""
        S, n = np.linalg.inv(self._D), self._dim
        E = [1.0 / S[i, i] for i in range(n)]
        if n == 2:
            return [E[0], E[1], -S[0, 1] * E[1], 1.0 / S[2, 2]]
        return [E[0], E[1], E[2], -S[0, 1] * E[1], -S[0, 2] * E[2], -S[1, 2] * E[2], 1.0 / S[3, 3], 1.0 / S[4, 4], 1.0 / S[5, 5]]

    def transform(self, R):
        """the tensor seen after rotating the material by the orthogonal ``R``: C'_ijkl = R_ip R_jq R_kr R_ls C_pqrs"""
        R = np.asarray(R, dtype=np.float64)
        n = self._dim
        if R.shape != (n, n) or np.abs(R @ R.T - np.eye(n)).max() > 1e-8:
            raise RuntimeError("transform needs an orthogonal %d x %d matrix" % (n, n))
        C = np.einsum("ip,jq,kr,ls,pqrs->ijkl", R, R, R, R, self.fullTensor())
        out = ElasticityTensor(dim=n)
        pr = _PAIRS[n]
        D = np.array([[C[a[0], a[1], b[0], b[1]] for b in pr] for a in pr])
        out._D, out._iso = 0.5 * (D + D.T), None
        return out


# ----------------------------------------------------------------------------------------------
# material files (Materials.cc:183-300)
# ----------------------------------------------------------------------------------------------

def _vector(entry, n):
    v = [float(x) for x in entry] if isinstance(entry, (list, tuple)) else None
    if v is None or len(v) != n:
        raise RuntimeError("Failed to parse vector of size %d" % n)
    return v


def _parse_orthotropic(m, t):
    if t.dim == 2:
        young, poisson, shear = _vector(m["young"], 2), _vector(m["poisson"], 2), _vector(m["shear"], 1)
        (Ex, Ey), (nu_xy, nu_yx) = young, poisson
        t.setOrthotropic(Ex, Ey, nu_yx, shear[0])
        bad = abs(nu_yx / Ey - nu_xy / Ex) > _SYM_TOL
    else:
        young, poisson, shear = _vector(m["young"], 3), _vector(m["poisson"], 6), _vector(m["shear"], 3)
        Ex, Ey, Ez = young
        nu_yz, nu_zy, nu_zx, nu_xz, nu_xy, nu_yx = poisson
        t.setOrthotropic(Ex, Ey, Ez, nu_yx, nu_zx, nu_zy, shear[0], shear[1], shear[2])
        bad = (abs(nu_yx / Ey - nu_xy / Ex) > _SYM_TOL or abs(nu_yz / Ey - nu_zy / Ez) > _SYM_TOL or
               abs(nu_zx / Ez - nu_xz / Ex) > _SYM_TOL)
    if bad:
        raise RuntimeError("Orthotopic parameters violate symmetry")         # (sic: the reference's message)


def _parse_anisotropic(m, t):
    rows = m["material_matrix"]
    n = _flat_len(t.dim)
    if not isinstance(rows, list) or len(rows) != n or any(not isinstance(r, list) or len(r) != n for r in rows):
        raise RuntimeError("Failed to parse material_matrix")
    t._D, t._iso = ElasticityTensor.fromD(rows, t.dim)._D, None


_PARSERS = {"isotropic_material": None, "isotropic": None,
            "orthotropic_material": _parse_orthotropic, "orthotropic": _parse_orthotropic,
            "symmetric_material": _parse_anisotropic, "anisotropic": _parse_anisotropic}


def read_material(path, dim):
    """the tensor of a material file for a ``dim``-dimensional simulator.  A tensor that is not positive definite is refused here,
    before anything reaches the device."""
    try:
        fh = open(path)
    except OSError:
        raise RuntimeError("Couldn't open material " + str(path))
    with fh:
        m = json.load(fh)
    kind = m.get("type", "isotropic_material")           # (a file without the key has always been read as isotropic here)
    if kind not in _PARSERS:
        raise RuntimeError("Invalid type.")
    t = ElasticityTensor(dim=dim)
    if _PARSERS[kind] is None:
        t.setIsotropic(float(m["young"]), float(m["poisson"]))
    else:
        _PARSERS[kind](m, t)
    require_positive_definite(t)
    return t


def require_positive_definite(t):
    if not np.all(np.isfinite(t._D)) or not t.isPositiveDefinite():
        raise RuntimeError("Elasticity tensor is not positive definite")
