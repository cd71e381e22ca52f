"""The frame layer of the read-count simulator, without a device: the output tables built by
index gather against a literal restatement of the reference's pivot / melt / merge rounds
(pert_simulator.py:336-418), the reference's helpers, and the seed rule."""
import numpy as np
import pandas as pd
import pytest
import torch
from pandas.testing import assert_frame_equal

from scdna_replication_tools.pert_simulator import (convert_rt_units, get_libraries_tensor, pert_simulator,
                                                     simulate_g_cells, simulate_s_cells)  # noqa: F401  the drop-in path
from scdna_replication_tools_amd import pert_simulator as ps

CLONES = ['B', 'A', 'C']
RT_COLS = ['rt_b', 'rt_a', 'rt_a']
CN_COL = 'true_somatic_cn'


def make_tables():
    """3 listed clones + one S cell of clone D, 2 libraries, chromosomes '1' (7 loci) and '10'
    (5 loci, listed first so the table's order differs from the pivot's), 9 S and 6 G cells, rows
    shuffled."""
    rng = np.random.default_rng(11)
    loci = [('10', 500 * i) for i in range(5)] + [('1', 1000 * i) for i in range(7)]
    gc = rng.uniform(0.3, 0.6, len(loci))
    rt_a, rt_b = rng.uniform(10, 80, len(loci)), rng.uniform(10, 80, len(loci))

    def table(cells, clone_of, suffix):
        rows = []
        for i, cell in enumerate(cells):
            for j, (c, s) in enumerate(loci):
                rows.append(dict(cell_id=cell, chr=c, start=s, end=s + 499, gc=gc[j], rt_a=rt_a[j], rt_b=rt_b[j],
                                 library_id='LIB{}'.format(i % 2), clone_id=clone_of[i],
                                 true_somatic_cn=float(1 + (i + j) % 4)))
        df = pd.DataFrame(rows)
        return df.sample(frac=1.0, random_state=3 + len(cells)).reset_index(drop=True)

    s_cells = ['s{:02d}'.format(i) for i in (7, 2, 5, 0, 8, 3, 1, 6, 4)]
    g_cells = ['g{:02d}'.format(i) for i in (3, 0, 5, 1, 4, 2)]
    df_s = table(s_cells, ['A', 'B', 'C', 'A', 'B', 'D', 'A', 'B', 'C'], 's')
    df_g = table(g_cells, ['A', 'B', 'C', 'A', 'B', 'C'], 'g')
    return df_s, df_g


def handmade_parts(df_s, df_g):
    """Fixed matrices in each clone's pivot shape."""
    s_parts = []
    for k, clone in enumerate(CLONES):
        sub = df_s.query('clone_id=="{}"'.format(clone))
        cn = pd.pivot_table(sub, index=['chr', 'start'], columns='cell_id', values=CN_COL)
        L, N = cn.shape
        base = np.arange(L * N, dtype=np.float64).reshape(L, N) + 1000 * k
        s_parts.append(((base * 3).astype(np.int64), base * 7 + 1, (base % 2), 1.0 / (2.0 + base),
                        (np.arange(N) + 1 + 10 * k).astype(np.float32) / 64))
    cn = pd.pivot_table(df_g, index=['chr', 'start'], columns='cell_id', values=CN_COL)
    base = np.arange(cn.size, dtype=np.float64).reshape(cn.shape) + 5000
    return s_parts, ((base * 2).astype(np.int64), base * 5 + 2)


def reference_frames(df_s, df_g, clones, s_parts, g_part, input_cn_col):
    """pert_simulator.py:336-418 with the simulated tensors replaced by the given matrices."""
    def melted(mat, cn, name):
        out = pd.DataFrame(mat, columns=cn.columns, index=cn.index)
        out = out.reset_index().melt(id_vars=['chr', 'start'], var_name='cell_id', value_name=name)
        out.chr = out.chr.astype(str)
        return out

    df_s_out = []
    for clone_id, (reads_norm, reads, rep, p_rep, t) in zip(clones, s_parts):
        clone_df_s = df_s.query('clone_id=="{}"'.format(clone_id))
        clone_cn_s = pd.pivot_table(clone_df_s, index=['chr', 'start'], columns='cell_id', values=input_cn_col)
        clone_t_df = pd.DataFrame(t, columns=['true_t'], index=clone_cn_s.columns)
        clone_df_s = pd.merge(clone_df_s, melted(reads_norm, clone_cn_s, 'true_reads_norm'))
        clone_df_s = pd.merge(clone_df_s, melted(reads, clone_cn_s, 'true_reads_raw'))
        clone_df_s = pd.merge(clone_df_s, melted(rep, clone_cn_s, 'true_rep'))
        clone_df_s = pd.merge(clone_df_s, melted(p_rep, clone_cn_s, 'true_p_rep'))
        clone_df_s = pd.merge(clone_df_s, clone_t_df.reset_index(), on='cell_id')
        df_s_out.append(clone_df_s)
    df_s = pd.concat(df_s_out, ignore_index=True)
    cn_g = pd.pivot_table(df_g, index=['chr', 'start'], columns='cell_id', values=input_cn_col)
    df_g = pd.merge(df_g, melted(g_part[0], cn_g, 'true_reads_norm'))
    df_g = pd.merge(df_g, melted(g_part[1], cn_g, 'true_reads_raw'))
    df_g['true_t'] = 0.0
    df_g['true_rep'] = 0.0
    df_g['true_p_rep'] = 0.0
    df_s['true_total_cn'] = df_s[input_cn_col] * (df_s['true_rep'] + 1)
    df_g['true_total_cn'] = df_g[input_cn_col] * (df_g['true_rep'] + 1)
    return df_s, df_g


def test_frames_match_the_reference_rounds():
    df_s, df_g = make_tables()
    s_parts, g_part = handmade_parts(df_s, df_g)
    want_s, want_g = reference_frames(df_s.copy(), df_g.copy(), CLONES, s_parts, g_part, CN_COL)
    got_s, got_g = ps.assemble_frames(df_s.copy(), df_g.copy(), CLONES, s_parts, g_part, CN_COL)
    assert_frame_equal(got_s, want_s)          # values, dtypes, column order, row order, index
    assert_frame_equal(got_g, want_g)
    assert 'D' not in set(got_s['clone_id']) and got_s['cell_id'].nunique() == 8
    assert got_s['true_reads_norm'].dtype == np.int64 and got_s['true_t'].dtype == np.float32
    assert list(got_s['clone_id'].drop_duplicates()) == CLONES


def test_pivot_matches_pivot_table():
    df_s, _ = make_tables()
    want = pd.pivot_table(df_s, index=['chr', 'start'], columns='cell_id', values=CN_COL)
    pv = ps.pivot(df_s, CN_COL)
    np.testing.assert_array_equal(pv.values, want.values)
    assert list(pv.cells) == list(want.columns)
    assert list(zip(pv.chr, pv.start)) == list(want.index)
    np.testing.assert_array_equal(pv.values[pv.li, pv.ci], df_s[CN_COL].to_numpy())
    # a per-locus column, looked up per locus of the pivot (not in order of first appearance)
    locus_gc = df_s.drop_duplicates(['chr', 'start']).set_index(['chr', 'start'])['gc']
    np.testing.assert_array_equal(pv.per_locus(df_s['gc'].to_numpy()), locus_gc.loc[list(want.index)].to_numpy())


def test_convert_rt_units():
    rt = np.array([3.0, 80.5, 41.25, 10.0, 80.5])
    want = 1 - ((rt - rt.min()) / (rt.max() - rt.min()))
    np.testing.assert_array_equal(convert_rt_units(rt), want)
    assert convert_rt_units(rt).min() == 0.0 and convert_rt_units(rt)[0] == 1.0      # the smallest value is the latest
    np.testing.assert_array_equal(convert_rt_units(pd.Series(rt)).to_numpy(), want)


def test_get_libraries_tensor():
    df_s, _ = make_tables()
    libs, n_libs = get_libraries_tensor(df_s)
    ref = df_s[['cell_id', 'library_id']].drop_duplicates()                # pert_simulator.py:184-196
    ids = ref['library_id'].unique()
    want = ref['library_id'].map({lib: i for i, lib in enumerate(ids)}).to_numpy()
    assert n_libs == 2 and libs.dtype == torch.int64 and libs.device.type == 'cpu'
    np.testing.assert_array_equal(libs.numpy(), want)


class FakeSampler:
    """Stands in for the device: records the seeds, returns matrices of the right shapes."""

    def __init__(self):
        self.calls = []

    def __call__(self, cn, gc, libs, n_libs, betas, u, lamb, seed, rho, a, num_reads, beta_stds, cell0, device):
        self.calls.append(dict(seed=seed, cell0=cell0, u=u, N=cn.shape[1], gc=np.array(gc),
                               rho=None if rho is None else np.array(rho)))
        z = np.zeros(cn.shape)
        if rho is None:
            return z.astype(np.int64), z, None, None, None
        return z.astype(np.int64), z, z, z, np.full(cn.shape[1], 0.5, np.float32)


def run_with_fake(monkeypatch, **kw):
    fake = FakeSampler()
    monkeypatch.setattr(ps, "_sample", fake)
    df_s, df_g = make_tables()
    out = pert_simulator(df_s, df_g, 5000, RT_COLS, CLONES, 0.75, [0.5, 0.0], 10.0, **kw)
    return fake, out, (df_s, df_g)


def test_seed_none_follows_torch_manual_seed(monkeypatch):
    torch.manual_seed(5)
    first, _, _ = run_with_fake(monkeypatch)
    second, _, _ = run_with_fake(monkeypatch)              # the generator has moved on
    torch.manual_seed(5)
    again, _, _ = run_with_fake(monkeypatch)
    seeds = lambda f: [c['seed'] for c in f.calls]
    assert len(set(seeds(first))) == 1                      # one seed per call of pert_simulator
    assert seeds(first) == seeds(again)
    assert seeds(first) != seeds(second)
    given, _, _ = run_with_fake(monkeypatch, seed=1234)
    assert seeds(given) == [1234] * 4


def test_simulator_arguments(monkeypatch):
    """What the sampler is asked for: global cell numbering, u per matrix, gc and rho per pivot locus."""
    fake, (out_s, out_g), (df_s, df_g) = run_with_fake(monkeypatch, seed=1)
    assert [c['cell0'] for c in fake.calls] == [0, 3, 6, 8] and [c['N'] for c in fake.calls] == [3, 3, 2, 6]
    L = 12
    for call, clone, rt_col in zip(fake.calls, CLONES, RT_COLS):
        sub = df_s.query('clone_id=="{}"'.format(clone))
        cn = pd.pivot_table(sub, index=['chr', 'start'], columns='cell_id', values=CN_COL)
        assert call['u'] == pytest.approx(5000 / (1.5 * L * cn.values.mean()), rel=1e-14)
        by_locus = sub.drop_duplicates(['chr', 'start']).set_index(['chr', 'start']).loc[list(cn.index)]
        np.testing.assert_array_equal(call['gc'], by_locus['gc'].to_numpy())
        np.testing.assert_array_equal(call['rho'], convert_rt_units(by_locus[rt_col].to_numpy()))
    cn_g = pd.pivot_table(df_g, index=['chr', 'start'], columns='cell_id', values=CN_COL)
    assert fake.calls[3]['u'] == pytest.approx(5000 / (L * cn_g.values.mean()), rel=1e-14)
    assert fake.calls[3]['rho'] is None
    assert len(out_s) == 8 * L and len(out_g) == 6 * L
    assert (out_g[['true_t', 'true_rep', 'true_p_rep']] == 0.0).all().all()
    assert list(out_s.columns[-6:]) == ['true_reads_norm', 'true_reads_raw', 'true_rep', 'true_p_rep', 'true_t',
                                        'true_total_cn']
    assert list(out_g.columns[-6:]) == ['true_reads_norm', 'true_reads_raw', 'true_t', 'true_rep', 'true_p_rep',
                                        'true_total_cn']
