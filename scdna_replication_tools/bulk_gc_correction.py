"""reference scdna_replication_tools/bulk_gc_correction.py (:21-74): reads per million, and the
bulk G1 GC correction by one LOWESS curve per library (scdna_replication_tools_amd.gc_correction)."""
from scdna_replication_tools_amd.gc_correction import (  # noqa: F401
    bulk_g1_gc_correction, compute_reads_per_million, predict_gc)
