"""Drop-in import path of the reference package (shahcompbio/scdna_replication_tools).

Notebooks and pipelines written against the reference import from here unchanged, e.g.
``from scdna_replication_tools.infer_scRT import scRT`` (inference_tutorial cell 1).  Each
module of this package is the reference module of the same name (file:line cited in
its docstring) and binds the MI355X implementation in ``scdna_replication_tools_amd``:
the PERT fits (steps 1-3, decode) run through libpert_hip.so on the GPU; there is no
CPU fallback.  Modules of the reference outside the PERT hot path (plotting, the
deterministic 'cell' / 'clone' levels, the SPF analysis) are not provided
(DESIGN.md section 8); the cell-cycle-classifier features are (``compute_ccc_features``,
DESIGN.md section 6j); the pseudobulk and T-width analyses of the decode are
(``compute_pseudobulk_rt_profiles``, ``calculate_twidth``), and so is the read-count simulator
upstream of the fit (``pert_simulator``: the reference's generative model drawn by a HIP
sampler).  ``scRT(..., posterior_draws=n)`` additionally leaves n posterior
draws of the S-phase states on ``scrt.model.draws_s`` (no reference counterpart beyond
``infer_discrete(temperature=1)``).
"""
