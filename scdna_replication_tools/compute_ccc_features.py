"""reference scdna_replication_tools/compute_ccc_features.py (:18-186): the cell-cycle-classifier
features (lrs, madn, breakpoints and their corrections), all cells of one length in one batched pass."""
from scdna_replication_tools_amd.ccc_features import (  # noqa: F401
    autocorr, breakpoints, calculate_breakpoints, calculate_features, compute_ccc_features, compute_cell_frac,
    compute_clone_normalization, compute_read_count, correct_breakpoints, correct_madn, get_args, main)
