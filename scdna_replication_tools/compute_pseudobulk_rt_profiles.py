"""reference scdna_replication_tools/compute_pseudobulk_rt_profiles.py (:16-69): population and
per-clone pseudobulk replication-timing profiles, computed from whole columns."""
from scdna_replication_tools_amd.rt_profiles import (  # noqa: F401
    calc_population_rt, compute_pseudobulk_rt_profiles)
