"""GPU: posterior marginals of replication and copy-number state (pert_enum_posterior,
PertShard.posterior, pert_infer_scRT(posterior=True)) against the fp64 oracle.

Every output element must lie within the derived bound of tests/_post_bounds.py of the
marginals of softmax(oracle.enum_scores) at the same point; the pass must agree with the decode
where the posterior is decisive, leave the padding and the fit's state untouched, and be
bit-identical from run to run.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _post_bounds as pb
from tests._problems import KIND_OF, init_constrained, make_problem

pytestmark = pytest.mark.gpu

# (kind, L, N, P, make_problem arguments)
CASES = {
    "step2_deep": ("step2", 40, 70, 13, dict(seed=0)),                       # second cell tile: 6 real lanes
    "step2_low": ("step2", 40, 70, 13, dict(seed=0, low_reads=True)),
    "step3_low": ("step3", 33, 65, 5, dict(seed=2, low_reads=True)),        # frozen rho / a; one real lane
    "bin_tiles": ("step2", 150, 64, 13, dict(seed=4, low_reads=True, prior="composite")),   # L > kMaxLT = 64
    "P16": ("step2", 24, 130, 16, dict(seed=7, low_reads=True, prior="uniform", z_scale=0.3)),
    "tiny": ("step2", 2, 1, 13, dict(seed=6, n_libs=1, low_reads=True)),
    "tiny_P2": ("step2", 2, 1, 2, dict(seed=5, K=2, n_libs=1)),              # smallest P and K, saturated
}
NONTRIVIAL = ("step2_deep", "step2_low", "step3_low", "bin_tiles", "P16")


@functools.lru_cache(maxsize=None)
def _case(name):
    """The problem, its oracle marginals (computed once, never modified) and the device run."""
    from scdna_replication_tools_amd.engine import PertShard
    kind, L, N, P, extra = CASES[name]
    while True:
        prob, kw, z = make_problem(kind, L=L, N=N, P=P, **extra)
        sh = PertShard(KIND_OF[kind], init=init_constrained(kind, z), device="cuda", dirichlet_mode="exact", **kw)
        if name != "bin_tiles" or -(-L // sh.bins_per_tile) >= 2:
            break
        L *= 2                                              # (cannot happen while tiles hold <= 64 bins)
    sh.set_unconstrained({k: v.numpy() for k, v in z.items()})
    ref = pb.oracle_marginals(prob, z)
    for v in ref.values():
        v.setflags(write=False)
    assert np.isfinite(ref["gamma"]).all()
    with_marg = {k: v.clone() for k, v in sh.posterior(cn_marginal=True).items()}
    cn_out, rep_out = sh.cn_out[:, :N].clone(), sh.rep_out[:, :N].clone()
    without = {k: v.clone() for k, v in sh.posterior().items()}
    torch.cuda.synchronize()
    return dict(prob=prob, z=z, sh=sh, ref=ref, with_marg=with_marg, without=without, cn_out=cn_out,
                rep_out=rep_out, L=L, N=N, P=P)


@pytest.mark.parametrize("name", list(CASES))
def test_marginals_within_bound_of_oracle(name):
    c = _case(name)
    ref, out = c["ref"], c["with_marg"]
    assert set(out) == {"rep_prob", "cn_prob", "cn_marg"} and set(c["without"]) == {"rep_prob", "cn_prob"}
    assert out["rep_prob"].shape == (c["L"], c["N"]) and out["cn_marg"].shape == (c["P"], c["L"], c["N"])
    r_rep = pb.check("rep_prob", out["rep_prob"].cpu().numpy(), ref["p_rep"], ref["b_rep"])
    r_cn = pb.check("cn_marg", out["cn_marg"].cpu().numpy(), ref["p_cn"], ref["b_cn"])
    # cn_prob: the oracle's marginal taken at the DEVICE's decoded state
    k = c["cn_out"].cpu().numpy().astype(np.int64)[None]
    r_cp = pb.check("cn_prob", out["cn_prob"].cpu().numpy(), np.take_along_axis(ref["p_cn"], k, 0)[0],
                    np.take_along_axis(ref["b_cn"], k, 0)[0])
    print("{}: worst |delta| / bound  rep {:.3f}  cn_marg {:.3f}  cn_prob {:.3f}; median bound {:.3g}; "
          "0.01 < P(rep) < 0.99 on {:.0%}".format(name, r_rep, r_cn, r_cp, float(np.median(ref["b_rep"])),
                                                  float(((ref["p_rep"] > 0.01) & (ref["p_rep"] < 0.99)).mean())))


@pytest.mark.parametrize("name", list(CASES))
def test_cn_prob_is_the_marginal_at_cn_out_and_cn_marg_is_optional(name):
    c = _case(name)
    a, b = c["with_marg"], c["without"]
    gathered = torch.gather(a["cn_marg"], 0, c["cn_out"].long()[None])[0]
    assert torch.equal(a["cn_prob"].view(torch.int32), gathered.view(torch.int32))
    assert torch.equal(a["rep_prob"].view(torch.int32), b["rep_prob"].view(torch.int32))
    assert torch.equal(a["cn_prob"].view(torch.int32), b["cn_prob"].view(torch.int32))
    # the pass's decode is the shard's decode
    cn, rep = c["sh"].decode()
    assert torch.equal(cn, c["cn_out"]) and torch.equal(rep, c["rep_out"])


@pytest.mark.parametrize("name", list(CASES))
def test_padding_untouched_and_reruns_bit_identical(name):
    """Through the C entry point on raw [L][ldn] / [P][L][ldn] buffers pre-filled with NaN:
    columns n < N finite and in [0, 1], columns n >= N still the fill's bit pattern; a second
    launch writes the same bytes."""
    c = _case(name)
    sh, L, N, P = c["sh"], c["L"], c["N"], c["P"]
    ldn = sh.ldn
    runs = []
    for _ in range(2):
        bufs = [torch.full(s, float("nan"), dtype=torch.float32, device=sh.device)
                for s in ((L, ldn), (L, ldn), (P, L, ldn))]
        fill = bufs[0].view(torch.int32)[0, 0].item()
        rc = sh.lib.pert_enum_posterior(ctypes.byref(sh._prob), ctypes.byref(sh._state), sh.cn_out.data_ptr(),
                                        bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), sh._stream())
        assert rc == 0
        torch.cuda.synchronize()
        for b in bufs:
            real, pad = b[..., :N], b[..., N:]
            assert torch.isfinite(real).all() and real.min() >= 0.0 and real.max() <= 1.0
            assert pad.numel() > 0 and (pad.contiguous().view(torch.int32) == fill).all()
        runs.append(bufs)
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(runs[0][0][:, :N].view(torch.int32), c["with_marg"]["rep_prob"].view(torch.int32))


@pytest.mark.parametrize("name", list(CASES))
def test_consistent_with_the_decode_where_decisive(name):
    """Where the oracle's top joint probability is >= 0.75 its score gap to every other state is
    >= log 3, far above the fp32 score error (E_s <= 0.12 on these shapes), so the decode is the
    oracle's there: rep_out is the side of 1/2 rep_prob lies on, and the decoded CN state's
    marginal is at least the joint's 0.75, within the bound."""
    c = _case(name)
    ref = c["ref"]
    P = c["P"]
    top = ref["gamma"].reshape((2 * P,) + ref["gamma"].shape[2:]).max(0)
    sel = top >= 0.75
    assert float(ref["E"].max()) < 0.5 * np.log(3.0)
    if name in NONTRIVIAL:
        assert sel.mean() >= 0.5, sel.mean()
    rep_prob = c["with_marg"]["rep_prob"].cpu().numpy()
    cn_prob = c["with_marg"]["cn_prob"].cpu().numpy()
    rep_out = c["rep_out"].cpu().numpy()
    k = c["cn_out"].cpu().numpy().astype(np.int64)[None]
    b_at = np.take_along_axis(ref["b_cn"], k, 0)[0]
    assert (rep_out[sel] == (rep_prob[sel] > 0.5)).all()
    assert (cn_prob[sel] >= 0.75 - b_at[sel]).all()
    print("{}: decisive on {:.0%}".format(name, float(sel.mean())))


@pytest.mark.parametrize("name", list(CASES))
def test_nothing_else_moves(name):
    c = _case(name)
    sh = c["sh"]
    loss0, _ = sh.loss_and_grads()
    cn0, rep0 = (t.clone() for t in sh.decode())
    z0, p0 = sh.z_pi.clone(), sh.params.clone()
    first = {k: v.clone() for k, v in sh.posterior(cn_marginal=True).items()}
    second = sh.posterior(cn_marginal=True)
    for k in first:
        assert torch.equal(first[k].view(torch.int32), second[k].view(torch.int32)), k
    assert torch.equal(sh.z_pi.view(torch.int32), z0.view(torch.int32))
    assert torch.equal(sh.params.view(torch.int32), p0.view(torch.int32))
    cn1, rep1 = sh.decode()
    assert torch.equal(cn1, cn0) and torch.equal(rep1, rep0)
    loss1, _ = sh.loss_and_grads()
    assert np.float64(loss0).tobytes() == np.float64(loss1).tobytes()


def test_step1_has_no_posterior():
    from scdna_replication_tools_amd.engine import PertShard
    prob, kw, z = make_problem("step1", L=8, N=6, seed=1)
    sh = PertShard(1, init=init_constrained("step1", z), device="cuda", **kw)
    with pytest.raises(ValueError):
        sh.posterior()


def test_pipeline_posterior_columns():
    """pert_infer_scRT(posterior=True) against posterior=False on the tables and limits of
    test_gpu_fit's pipeline test: everything that exists today is unchanged, and the two new
    columns are probabilities consistent with the calls."""
    import pandas as pd
    from scdna_replication_tools_amd.pert_model import pert_infer_scRT
    from scdna_replication_tools_amd.simulator import simulate, to_long_form
    sim = simulate(n_s=40, n_g=40, n_bins=300, num_reads=183 * 300, seed=2)
    df_s, df_g = to_long_form(sim, n_libs=1)
    runs = {}
    for flag in (False, True):
        m = pert_infer_scRT(df_s.copy(), df_g.copy(), input_col='reads', clone_col='clone_id',
                            cn_prior_method='g1_clones', max_iter=300, min_iter=50, rel_tol=1e-6, max_iter_step1=200,
                            max_iter_step3=100, posterior=flag)
        runs[flag] = m.run_pert_model()
    new = ["model_rep_prob", "model_cn_prob"]
    for i in (0, 2):                                        # the S output and step 3's G1/2 output
        plain, post = runs[False][i], runs[True][i]
        assert list(post.columns) == list(plain.columns) + new
        pd.testing.assert_frame_equal(post[list(plain.columns)], plain)
        for col in new:
            v = post[col].to_numpy()
            assert v.dtype == np.float32 and not np.isnan(v).any() and v.min() >= 0.0 and v.max() <= 1.0
        # P(cn call) >= 3/4 and P(rep = r) >= 3/4 for one r put >= 1/2 on the joint state
        # (call, r), which is then the MAP state: a theorem only with BOTH conditions
        rp = post["model_rep_prob"].to_numpy()
        sel = (post["model_cn_prob"].to_numpy() >= 0.75) & (np.abs(rp - 0.5) >= 0.25)
        assert sel.mean() > 0.5
        assert (post["model_rep_state"].to_numpy()[sel] == (rp[sel] > 0.5)).all()
    for i in (1, 3):
        pd.testing.assert_frame_equal(runs[True][i], runs[False][i])
