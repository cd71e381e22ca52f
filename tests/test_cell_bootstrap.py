"""CellBootstrap on the host: every replicate against RTMatrix run on the matrix whose columns are
the original's cells, each repeated w[n] times (the definition: exact, no tolerance), the
resampler against an independent Philox, and the calibration of the reported spread."""
import numpy as np
import pytest

from scdna_replication_tools_amd import cell_bootstrap as cb
from scdna_replication_tools_amd import rt_profiles as rt
from tests import _sim_ref as sr
from tests._rt_cases import same_bits


def matrix(L, N, seed=0, clones=True, p=0.45):
    rng = np.random.default_rng(seed)
    rep = (rng.uniform(size=(L, N)) < p).astype(np.uint8)
    clone_ids = None
    if clones:                                                  # three clones and cells without one
        clone_ids = np.array(["b", "a", "c", None], object)[np.arange(N) % 4]
    return rt.RTMatrix(rep, cell_ids=np.array(["c%03d" % ((7 * i) % N) for i in range(N)]),
                       chr=np.array(["2", "10", "1"])[np.arange(L) % 3], start=np.arange(L)[::-1].copy(),
                       clone_ids=clone_ids, device="cpu")


def repeated(m, w):
    """The RTMatrix whose columns are m's cells, each repeated w[n] times."""
    cols = np.repeat(np.arange(m.N), w)
    return rt.RTMatrix(m._rep_host[:, cols], cell_ids=m.cell_ids[cols], chr=m.chr, start=m.start,
                       clone_ids=None if m.clone_ids is None else m.clone_ids[cols], device="cpu")


def explicit_weights(N, B=4, seed=1):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 4, (B, N))
    w[0, 0], w[1, N - 1] = 255, 0
    return w


def assert_replicates_are_repeated_columns(m, boot, dtype, frac_dtype, loci):
    counts, size = boot.counts('clone')
    values, hours = boot.profiles('clone', dtype)
    pop_values, pop_hours = boot.profiles('population', dtype)
    kw = dict(dtype=dtype, frac_dtype=frac_dtype, loci=loci)
    hist_pop = boot.tfs_counts(by='population', **kw)
    hist_clone = boot.tfs_counts(by='clone', **kw)
    order = m.locus_order
    for b in range(len(boot)):
        w = boot.weights[b]
        o = repeated(m, w)
        o_count, _ = o.counts()
        pb = o.pseudobulk(dtype)
        assert counts[b].sum() == o_count.sum()
        assert same_bits(pop_values[b, 0][order], pb["population"][0])
        assert same_bits(pop_hours[b, 0][order], pb["population"][1])
        want = o.tfs_counts(by='population', **kw)
        assert (hist_pop[0][b, 0] == want[0]).all() and (hist_pop[1][b, 0] == want[1]).all()
        for g in range(len(m.clones) + 1):
            mine = m._clone_of == (g if g < len(m.clones) else -1)
            assert size[b, g] == w[mine].sum()
            if g == len(m.clones):
                assert (counts[b, g] == o_count[-1]).all()
                continue
            c = m.clones[g]
            if c not in pb["clones"]:                           # the replicate holds no cell of this clone
                assert size[b, g] == 0 and not counts[b, g].any() and np.isnan(values[b, g]).all()
                assert not hist_clone[0][b, g].any() and not hist_clone[1][b, g].any()
                continue
            assert (counts[b, g] == o_count[list(o.clones).index(c)]).all()
            assert same_bits(values[b, g][order], pb["clones"][c][0])
            assert same_bits(hours[b, g][order], pb["clones"][c][1])
            want = o.tfs_counts(by='clone', cells=m.cell_ids[mine], **kw)
            assert (hist_clone[0][b, g] == want[0]).all() and (hist_clone[1][b, g] == want[1]).all()
        assert hist_pop[0][b].sum() > 0


@pytest.mark.parametrize("dtype,frac_dtype", [(np.float32, np.float32), (np.float32, np.float64),
                                              (np.float64, np.float64)])
@pytest.mark.parametrize("generated", [False, True])
@pytest.mark.parametrize("L,N", [(7, 5), (65, 37)])
def test_oracle_identity(L, N, generated, dtype, frac_dtype):
    m = matrix(L, N)
    boot = m.bootstrap(n_boot=4, seed=11) if generated else cb.CellBootstrap(m, weights=explicit_weights(N))
    assert boot.weights.dtype == np.uint8 and boot.weights.shape == (4, N)
    loci = None if dtype == np.float32 else (m.chr != "10")    # a mask, as query2 restricts the rows
    assert_replicates_are_repeated_columns(m, boot, dtype, frac_dtype, loci)


def test_host_weights_are_the_documented_philox_draws():
    strata = np.array([2, 0, 1, 2, 2, 0, 2, 1, 2, 2, 0])
    seed, b0, B = (7 << 33) + 12345, (1 << 32) + 5, 3
    got = cb.boot_weights_host(strata, B, seed=seed, b0=b0)
    order = sorted(range(len(strata)), key=lambda n: (strata[n], n))
    want = np.zeros((B, len(strata)), np.int64)
    for r in range(B):
        b = b0 + r
        for j, n in enumerate(order):
            members = [c for c in order if strata[c] == strata[n]]
            w = sr.philox(np.array([j, b & 0xFFFFFFFF, 4, b >> 32], np.uint32), sr.make_key(seed, 4))
            word = (int(w[1]) << 32) | int(w[0])
            want[r, members[(word * len(members)) >> 64]] += 1
    assert (got == want).all()


def test_every_stratum_keeps_its_size():
    m = matrix(7, 37)
    boot = m.bootstrap(n_boot=6, seed=3)
    for g in range(4):
        mine = m._clone_of == (g if g < 3 else -1)
        assert (boot.weights[:, mine].sum(axis=1) == mine.sum()).all()
    one = matrix(7, 37, clones=False).bootstrap(n_boot=6, seed=3)
    assert (one.weights.sum(axis=1) == 37).all()
    assert not (one.weights == boot.weights).all()


def test_seed_and_chunking():
    m = matrix(65, 37)
    a, b = m.bootstrap(n_boot=3, seed=5), m.bootstrap(n_boot=8, seed=5)
    assert (a.weights == b.weights[:3]).all()
    assert not (b.weights == m.bootstrap(n_boot=8, seed=6).weights).all()
    ref = b.counts('clone'), b.tfs_counts(by='clone')
    for chunk in (1, 3, 8):
        c = m.bootstrap(n_boot=8, seed=5, chunk=chunk)
        assert (c.weights == b.weights).all()
        got = c.counts('clone'), c.tfs_counts(by='clone')
        for x, y in zip(ref[0] + ref[1], got[0] + got[1]):
            assert x.dtype == np.int64 and same_bits(x, y)


def test_edge_rows():
    m = matrix(65, 37)
    w = np.ones((2, 37), np.int64)
    w[1, m._clone_of == 1] = 0                                  # replicate 1 holds no cell of clone 'b'
    w[0, 3] = 255
    boot = cb.CellBootstrap(m, weights=w)
    values, hours = boot.profiles('clone')
    assert np.isnan(values[1, 1]).all() and np.isnan(hours[1, 1]).all() and not np.isnan(values[0]).any()
    hn, hr = boot.tfs_counts(by='clone')
    assert not hn[1, 1].any() and not hr[1, 1].any() and hn[0, 1].any()
    assert_replicates_are_repeated_columns(m, boot, np.float32, np.float32, None)
    for bad in (np.full((2, 37), 256), np.full((2, 37), -1), np.ones((2, 36), int), np.ones(37, int),
                np.ones((2, 37), float)):
        with pytest.raises(ValueError):
            cb.CellBootstrap(m, weights=bad)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hours_twin(dtype):
    rng = np.random.default_rng(2)
    rows = rng.integers(0, 50, (12, 33)).astype(dtype) / dtype(50)
    rows[3] = dtype(0.25)                                       # constant: NaN
    rows[5] = np.nan
    rows[7] = 0
    rows = rows.reshape(3, 4, 33)
    got = cb._hours_from_profiles(rows)
    assert got.dtype == dtype and got.shape == rows.shape
    for i in range(3):
        for j in range(4):
            assert same_bits(got[i, j], rt._hours_from_profile(rows[i, j]))
    assert np.isnan(got[0, 3]).all() and np.isnan(got[1, 1]).all() and got[0, 0].max() == 10


def test_frames():
    m = matrix(65, 37, seed=4)
    boot = m.bootstrap(n_boot=5, seed=1)
    pb = boot.pseudobulk()
    stats = ["mean", "q5", "q50", "q95", "sd"]
    want = ["chr", "start"] + ["pseudobulk_" + s for s in stats]
    for c in ("a", "b", "c"):
        want += ["pseudobulk_clone{}_{}".format(c, s) for s in stats]
    assert list(pb.columns) == want and len(pb) == 65
    own = m.pseudobulk_frame()
    assert (pb["chr"] == own["chr"]).all() and (pb["start"] == own["start"]).all()
    assert (pb["pseudobulk_q5"] <= pb["pseudobulk_q95"]).all() and (pb["pseudobulk_sd"] >= 0).all()
    tw = boot.twidth(curve="linear")
    assert list(tw.columns) == ["replicate", "t_width", "right_time", "left_time", "popt_0", "popt_1"]
    assert list(tw["replicate"]) == list(range(5))
    per = boot.twidth(curve="linear", per_clone=True)
    assert list(per.columns) == ["replicate", "clone_id", "t_width", "right_time", "left_time", "popt_0", "popt_1"]
    assert list(per["replicate"]) == [b for b in range(5) for _ in range(3)]
    assert list(per["clone_id"]) == ["a", "b", "c"] * 5
    iv = boot.twidth_interval(curve="linear")
    assert list(iv.columns) == ["t_width", "t_width_mean", "t_width_q5", "t_width_q50", "t_width_q95", "t_width_sd"]
    assert len(iv) == 1 and iv["t_width"][0] == m.twidth(curve="linear")[0]
    assert iv["t_width_mean"][0] == tw["t_width"].mean()
    ivc = boot.twidth_interval(curve="linear", per_clone=True, q=(0.5,))
    assert list(ivc.columns) == ["clone_id", "t_width", "t_width_mean", "t_width_q50", "t_width_sd"]
    assert list(ivc["clone_id"]) == ["a", "b", "c"]


def test_calibration():
    """iid Bernoulli(p) cells: the bootstrap sd of a bin's pseudobulk mean estimates
    sqrt(p (1 - p) / N).  A sample sd over B replicates has relative standard deviation
    1 / sqrt(2 (B - 1)); the bound is six of those."""
    p, N, L, B = 0.3, 400, 64, 400
    m = matrix(L, N, seed=9, clones=False, p=p)
    sd = m.bootstrap(n_boot=B, seed=2).pseudobulk()["pseudobulk_sd"].to_numpy().mean()
    want = np.sqrt(p * (1 - p) / N)
    assert abs(sd / want - 1) < 6 / np.sqrt(2 * (B - 1)), (sd, want)
