"""reference scdna_replication_tools/pert_simulator.py (:177-418): the read-count simulator,
its draws made by the HIP sampler (csrc/sim_kernels.hip) instead of a Pyro trace."""
from scdna_replication_tools_amd.pert_simulator import (  # noqa: F401
    convert_rt_units, get_libraries_tensor, pert_simulator, simulate_g_cells, simulate_s_cells)
