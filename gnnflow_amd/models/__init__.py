"""The reference's model package (gnnflow/models): `from gnnflow_amd.models.dgnn import DGNN` and
the `models.modules.{layers,memory,memory_updater}` import lines work with the package name
swapped."""
from .dgnn import DGNN

__all__ = ["DGNN"]
