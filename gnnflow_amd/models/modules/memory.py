"""gnnflow/models/modules/memory.py: gnnflow_amd.memory.Memory under the reference's name."""
from ...memory import Memory  # noqa: F401
