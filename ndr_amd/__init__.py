"""MI355X-native voxel-FEM topology-optimization hot path (drop-in for the `pyVoxelFEM` surface of
Nikronic/ndr).  See DESIGN.md for scope and INTEGRATION.md for the reference-side binding."""
__version__ = "0.1.0"

from .materials import ElasticityTensor  # noqa: E402,F401  (numpy only: importing the package still loads neither torch nor the library)
