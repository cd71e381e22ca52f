"""reference scdna_replication_tools/normalize_by_clone.py (:22-77): S-phase profiles divided by
their clone's consensus profile, computed from whole columns."""
from scdna_replication_tools_amd.binarize import cell_clone_norm, normalize_by_clone  # noqa: F401
