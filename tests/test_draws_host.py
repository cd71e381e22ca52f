"""Posterior draws of the enumerated states without a GPU: the per-element arithmetic (pert_math.h
enum_draw_cdf / enum_draw_pick, compiled for the host) against the fp64 reference within the
conditions of tests/_draw_ref.py, the argument checks of pert_enum_draw, and the public keywords.
"""
import ctypes
import inspect

import numpy as np
import pytest

from tests import _draw_ref as dr
from tests.test_posterior_host import LAM, _inputs, _problem, _reference, _tables

N_DRAWS = 8
SEED = 11


@pytest.fixture(scope="module")
def nat():
    from scdna_replication_tools_amd import build, _native
    build.build()
    _native.lib()
    return _native


def _elements(P):
    """test_posterior_host's 300 elements (x = 0 rows, phi outside its clamps, saturated logits)
    with the last one replaced by a row whose last states underflow in fp32: no reads at D = 60,
    so every state with chi >= 2 scores about 166 (chi - 1) below the state chi = 0."""
    x, z, D, phi = _inputs(P)
    x[-1], D[-1], phi[-1] = 0.0, 60.0, 0.5
    z[-1] = 0.0
    return x, z, D, phi


@pytest.mark.parametrize("P", [2, 5, 13, 16])
def test_enum_draw_host_within_oracle_condition(nat, P):
    x, z, D, phi = _elements(P)
    n = x.size
    ref, _ = _reference(P, x, z, D, phi)
    g = dr.joint_order(ref["gamma"])
    assert (x == 0).sum() >= 10 and ((phi < 0.001) | (phi > 0.999)).sum() >= 10
    assert g[-1, -1] < dr.ZERO_WEIGHT * 2 * P and g[-1, -1] < g[0, -1]      # the underflowing row
    # element i is (bin 0, global cell i) of the counter rule
    u = dr.uniforms(SEED, 0, np.arange(n), 0, N_DRAWS)                       # (n_draws, n)
    out = nat.selftest_enum_draw_host(P, x, z, np.log1p(-LAM), D, phi, u.T)
    assert out["cn"].shape == (n, N_DRAWS) and out["cn"].dtype == np.uint8 and out["rep"].max() <= 1
    j_dev = 2 * out["cn"].astype(np.int64).T + out["rep"].T
    share = dr.check("P={}".format(P), ref, u, j_dev)
    _, _, b = dr.prefix(ref)
    print("P={}: {:.3%} of {} draws differ from the fp64 draw (cap {:.0%}); median prefix bound {:.3g}".format(
        P, share, j_dev.size, dr.CAP, float(np.median(b))))
    # the test has power: both rep states and several cn states are drawn, and uncertain elements exist
    assert (out["rep"] == 1).any() and (out["rep"] == 0).any() and np.unique(out["cn"]).size > 1
    top = g.max(0)
    assert (top < 0.99).mean() > 0.1


def test_enum_draw_host_extreme_uniforms(nat):
    """u next to 0 takes the first state with weight, u next to 1 the last one: never a state
    whose weight underflowed (the underflowing row's last states)."""
    P = 13
    x, z, D, phi = _elements(P)
    ref, _ = _reference(P, x, z, D, phi)
    g = dr.joint_order(ref["gamma"])
    u = np.tile(np.array([2.0 ** -25, 1.0 - 2.0 ** -24], np.float32), (x.size, 1))
    out = nat.selftest_enum_draw_host(P, x, z, np.log1p(-LAM), D, phi, u)
    j = 2 * out["cn"].astype(np.int64) + out["rep"]
    assert (np.take_along_axis(g, j.T, 0) >= dr.ZERO_WEIGHT * 2 * P).all()
    assert j[-1, 1] < 2 * P - 1 and (j[:, 0] <= j[:, 1]).all()


def test_enum_draw_abi_and_argument_checks(nat):
    """Both names are exported and every argument error returns before any launch (no GPU
    here): the pointers below are host buffers that are never dereferenced."""
    assert {"pert_enum_draw", "pert_selftest_enum_draw_host"} <= set(nat.EXPORTED_SYMBOLS)
    lib = nat.lib()
    assert hasattr(lib, "pert_enum_draw") and hasattr(lib, "pert_selftest_enum_draw_host")
    assert nat.TAG_DRAWS == 3 and nat.TAG_DRAWS not in (nat.SIM_TAG_CELLS, nat.SIM_TAG_READS)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    st = nat.PertState(params=p, z_pi=p)

    def call(pr, rep=p, cn=p, first=0, n=8, cell0=0, state=st):
        return lib.pert_enum_draw(ctypes.byref(pr), ctypes.byref(state), 1, cell0, first, n, rep, cn, None)

    good = dict(reads=p, gcf=p)
    E_ARG, E_P, E_K = 1, 2, 3
    assert call(_problem(nat, **good), rep=None) == E_ARG                      # null rep_draw
    assert call(_problem(nat, **good), rep=None, cn=None) == E_ARG
    assert call(_problem(nat, kind=1, **good)) == E_ARG                        # step 1
    assert call(_problem(nat, P=17, **good)) == E_P
    assert call(_problem(nat, P=1, **good)) == E_P
    assert call(_problem(nat, K1=9, **good)) == E_K
    assert call(_problem(nat, L=0, **good)) == E_ARG
    assert call(_problem(nat, ldn=100, **good)) == E_ARG                       # not a multiple of PERT_BLOCK
    assert call(_problem(nat, N=300, **good)) == E_ARG                         # ldn < N
    assert call(_problem(nat, N=0, **good)) == E_ARG
    assert call(_problem(nat)) == E_ARG                                        # null reads / gcf
    assert call(_problem(nat, **good), state=nat.PertState(params=p)) == E_ARG  # null z_pi
    assert call(_problem(nat, kind=3, **good)) == E_ARG                        # step 3 without rho_fixed
    # the order of pert_enum_posterior's checks: the shape before P, P before K1, K1 before the pointers
    assert call(_problem(nat, L=0, P=17, **good)) == E_ARG
    assert call(_problem(nat, P=17, K1=9)) == E_P
    assert call(_problem(nat, K1=9)) == E_K
    for n in (0, -1, nat.MAX_DRAWS + 1):
        assert call(_problem(nat, **good), n=n) == E_ARG                       # n_draws outside [1, 4096]
    assert call(_problem(nat, **good), first=-1) == E_ARG
    assert call(_problem(nat, **good), first=2 ** 31 - 8, n=9) == E_ARG        # first_draw + n_draws overflows
    assert call(_problem(nat, **good), cell0=-1) == E_ARG
    assert call(_problem(nat, **good, L=65536 * 64 + 1)) == E_ARG              # more than 65535 bin tiles
    assert lib.pert_enum_draw(None, ctypes.byref(st), 1, 0, 0, 8, p, p, None) == E_ARG
    assert lib.pert_enum_draw(ctypes.byref(_problem(nat, **good)), None, 1, 0, 0, 8, p, p, None) == E_ARG
    assert lib.pert_selftest_enum_draw_host(17, 0, None, None, 0.0, None, None, 1, None, None, None) == E_P
    assert lib.pert_selftest_enum_draw_host(13, 0, None, None, 0.0, None, None, 0, None, None, None) == E_ARG


def test_constructor_takes_draw_keywords_only():
    from scdna_replication_tools_amd.pert_model import pert_infer_scRT
    params = inspect.signature(pert_infer_scRT.__init__).parameters
    for name, default in (("posterior_draws", 0), ("draws_seed", None)):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default == default
    m, _, _, _ = _tables()
    assert m.posterior_draws == 0 and m.draws_s is None
    kw = dict(input_col='reads', clone_col='clone_id', cn_prior_method='g1_clones', device='cpu')
    a = pert_infer_scRT(m.cn_s, m.cn_g1, seed=5, posterior_draws=3, **kw)
    assert a.posterior_draws == 3 and a.draws_seed == 5                       # draws_seed None means seed
    assert pert_infer_scRT(m.cn_s, m.cn_g1, seed=5, posterior_draws=3, draws_seed=2 ** 40, **kw).draws_seed == 2 ** 40
    for bad in (-1, 4097):
        with pytest.raises(ValueError):
            pert_infer_scRT(m.cn_s, m.cn_g1, posterior_draws=bad, **kw)
    with pytest.raises(TypeError):
        pert_infer_scRT(m.cn_s, m.cn_g1, *([None] * 29), 4)                   # not positional


def test_default_leaves_package_s_output_columns():
    """posterior_draws does not reach package_s_output: its columns are today's, with and
    without the keyword."""
    from scdna_replication_tools_amd.pert_model import MapTrace, PivotAxes, pert_infer_scRT
    m, _, tr, _ = _tables()
    lam, lg, ls = np.array([0.71], np.float32), [3.0, 2.0], [9.0]
    want = list(m.cn_s.columns) + ["model_cn_state", "model_rep_state", "model_tau", "model_u", "model_rho"]
    for model in (m, pert_infer_scRT(m.cn_s, m.cn_g1, input_col='reads', clone_col='clone_id',
                                     cn_prior_method='g1_clones', device='cpu', posterior_draws=4)):
        inp = model._prepare()
        axes = PivotAxes(inp.loci_chr, inp.loci_start, inp.cells_s, keys=inp.keys_s)
        got, _ = model.package_s_output(model.cn_s, MapTrace(**tr), axes, lam, lg, ls)
        assert list(got.columns) == want
