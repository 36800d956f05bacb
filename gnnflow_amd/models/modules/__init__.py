"""gnnflow/models/modules under its own module names; the classes live in gnnflow_amd.nn and
gnnflow_amd.memory."""
