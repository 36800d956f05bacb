"""gnnflow/models/modules/memory_updater.py: nn.GRUMemoryUpdater under the reference's names."""
from ...nn import GRUMemeoryUpdater, GRUMemoryUpdater  # noqa: F401
