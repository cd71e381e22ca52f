"""reference scdna_replication_tools/normalize_by_cell.py: the deterministic cell level's
normalisation.  ``compute_cell_corrs`` (:148-180) is the S-cell vs G1-cell Pearson table the
correlation-matched CN priors rank; ``normalize_by_cell`` (:216-267) and its parts
(``g1_cell_norm``, ``remove_cell_specific_CNAs``, ``identify_changepoint_segs``,
``sort_by_cell_and_loci``) run the reference's change-point loop on a closed-form search
(scdna_replication_tools_amd/normalize_cell.py) instead of ruptures.  The argument parser and
``main`` (the command line) are not part of this build."""
from scdna_replication_tools_amd.normalize_cell import (  # noqa: F401
    g1_cell_norm, identify_changepoint_segs, normalize_by_cell, remove_cell_specific_CNAs, sort_by_cell_and_loci)
from scdna_replication_tools_amd.prep import compute_cell_corrs  # noqa: F401

__all__ = ["compute_cell_corrs", "g1_cell_norm", "identify_changepoint_segs", "normalize_by_cell",
           "remove_cell_specific_CNAs", "sort_by_cell_and_loci"]
