"""gnnflow/models/modules/layers.py: the classes of gnnflow_amd.nn under the reference's names."""
from ...nn import (MLP, EdgePredictor, TemporalAttentionLayer, TimeEncode,  # noqa: F401
                   TransfomerAttentionLayer)
