"""MI355X-native voxel-FEM topology-optimization hot path (drop-in for the `pyVoxelFEM` surface of
Nikronic/ndr).  See DESIGN.md for scope and INTEGRATION.md for the reference-side binding."""
__version__ = "0.1.0"

from .materials import ElasticityTensor  # noqa: E402,F401  (numpy only: importing the package still loads neither torch nor the library)

_LAZY = ("stress", "mma", "modal", "buckling", "loadcases", "thermal", "thermoelastic") # modules that load torch and the library: imported on first use, so that `import ndr_amd` stays light


def __getattr__(name):
    if name in _LAZY:
        import importlib
        return importlib.import_module("." + name, __name__)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def __dir__():
    return sorted(list(globals()) + list(_LAZY))
