"""reference scdna_replication_tools/calculate_twidth.py (:23-200): time from scheduled
replication, its 200-interval histogram and the T-width of the fitted curve."""
from scdna_replication_tools_amd.rt_profiles import (  # noqa: F401
    calc_linear_t_width, calc_pct_replicated_per_time_bin, calc_t_width, calculate_twidth,
    compute_and_plot_twidth, compute_time_from_scheduled_column, fit_linear, fit_sigmoid, inv_linear,
    inv_sigmoid, linear, plot_cell_variability, sigmoid)
