"""reference scdna_replication_tools/binarize_rt_profiles.py (:22-121): threshold binarisation of
RT profiles (Dileep & Gilbert), all cells of one length in one batched pass."""
from scdna_replication_tools_amd.binarize import binarize_profiles  # noqa: F401
