"""The reference's model package (gnnflow/models): `from gnnflow_amd.models.dgnn import DGNN`,
`from gnnflow_amd.models.graphsage import SAGE`, `from gnnflow_amd.models.gat import GAT` and the
`models.modules.{layers,memory,memory_updater}` import lines work with the package name
swapped.  GraphMixer and DyGFormer are this project's own additions, on the edge-history readers
of DynamicGraph instead of sampled blocks."""
from .dgnn import DGNN
from .dygformer import DyGFormer
from .gat import GAT
from .graphmixer import GraphMixer
from .graphsage import SAGE

__all__ = ["DGNN", "DyGFormer", "GAT", "GraphMixer", "SAGE"]
