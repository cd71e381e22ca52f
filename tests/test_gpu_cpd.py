"""pert_cpd_search (csrc/cpd_kernels.hip) on the GPU against its numpy twin cpd_search_host, bit for
bit on the breakpoints and on the gain (as uint64 patterns): ragged launches with both modes and
inactive cells, the full LDS budget, many cells, tie-heavy profiles, reruns; and normalize_by_cell on
the device against the reference fixture."""
import warnings

import numpy as np
import pytest

from scdna_replication_tools_amd import _native
from scdna_replication_tools_amd import normalize_cell as NC
from tests import _cell_cases as CC

pytestmark = pytest.mark.gpu


def _same(got, want, active=None):
    rows = slice(None) if active is None else np.flatnonzero(active)
    for g, w, name in zip(got, want, ("a", "b", "gain")):
        if name == "gain":
            assert (CC.bits(g[rows]) == CC.bits(w[rows])).all(), name
        else:
            assert g.dtype == np.int32 and (g[rows] == w[rows]).all(), (name, g[rows], w[rows])


def test_ragged_launch_mixed_modes_and_inactive_cells():
    rng = np.random.default_rng(21)
    sizes = [6, 7, 63, 64, 65, 257, 300] * 3 + [3, 4, 5, 5]
    profiles = [CC.noisy_steps(rng, n) for n in sizes]
    Y, lens = CC.ragged(profiles)
    mode = np.array([1 + (i % 2) for i in range(len(sizes))], np.int32)
    mode[:7] = 2
    mode[7:14] = 1
    active = np.ones(len(sizes), np.int32)
    active[[2, 9, 16]] = 0
    got = NC.cpd_search(Y, lens, mode, active)
    want = NC.cpd_search_host(Y, lens, mode, active)
    _same(got, want)                                  # inactive rows: -1, -1, NaN on both
    assert (got[0][np.array(active, bool) & (lens < 4)] == -1).all()
    for i in (0, 1, 7, 8):                            # and the twin is the definition
        assert (want[0][i], want[1][i]) == CC.triple_loop(profiles[i], int(mode[i]))[:2]


def test_inactive_outputs_are_left_as_they_are():
    rng = np.random.default_rng(22)
    Y, lens = CC.ragged([CC.noisy_steps(rng, 40) for _ in range(5)])
    s = NC._DeviceSearch(Y, "cuda")
    mode = np.full(5, 2, np.int32)
    first = s(lens, mode, np.ones(5, np.int32))
    s.update_rows([1], (Y[1] * 0.0)[None, :])
    second = s(lens, mode, np.array([0, 1, 0, 0, 0], np.int32))
    assert (second[0][1], second[1][1], second[2][1]) == (2, 4, 0.0)
    keep = [0, 2, 3, 4]
    _same([v[keep] for v in second], [v[keep] for v in first])


@pytest.mark.parametrize("n", [5451, _native.CPD_MAX_N])
def test_one_cell_at_the_lds_budget(n):
    """5,451 bins: the genome at 500 kb, more tiles of a than CUs for the one cell; CPD_MAX_N: the
    largest profile the entry point accepts."""
    rng = np.random.default_rng(n)
    y = CC.noisy_steps(rng, n, n_steps=4)
    for mode in (2, 1):
        _same(NC.cpd_search(y, mode=mode), NC.cpd_search_host(y, mode=mode))
    with pytest.raises(ValueError, match="exceeds"):
        NC.cpd_search(np.zeros(_native.CPD_MAX_N + 1))


def test_many_cells():
    rng = np.random.default_rng(23)
    Y = np.stack([CC.noisy_steps(rng, 271) for _ in range(300)])
    _same(NC.cpd_search(Y), NC.cpd_search_host(Y))
    _same(NC.cpd_search(Y, mode=1), NC.cpd_search_host(Y, mode=1))


def test_tie_order():
    """Profiles of a few repeated integers: many candidates with equal or nearly equal gains."""
    rng = np.random.default_rng(24)
    profiles = [rng.integers(0, 3, n).astype(np.float64) for n in (30, 64, 129, 300, 300, 513)]
    profiles += [np.zeros(300), np.ones(257), np.tile([1.0, -1.0], 100), np.repeat([2.0, 5.0, 2.0], 50)]
    Y, lens = CC.ragged(profiles)
    for mode in (2, 1):
        got, want = NC.cpd_search(Y, lens, mode), NC.cpd_search_host(Y, lens, mode)
        _same(got, want)
    a, b, g = NC.cpd_search(Y, lens, 2)
    assert (a[6], b[6], g[6]) == (2, 4, 0.0)          # all zeros: the smallest a, then the smallest b
    assert (a[9], b[9]) == (50, 100)


def test_two_launches_are_byte_identical():
    rng = np.random.default_rng(25)
    Y, lens = CC.ragged([CC.noisy_steps(rng, n) for n in (300, 271, 5451, 64, 1000)])
    mode = np.array([2, 1, 2, 2, 1], np.int32)
    first, second = NC.cpd_search(Y, lens, mode), NC.cpd_search(Y, lens, mode)
    for u, v in zip(first, second):
        assert u.tobytes() == v.tobytes()


def test_normalize_by_cell_on_the_device_equals_the_reference_module():
    fx = CC.fixture()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        out = NC.normalize_by_cell(CC.frame(fx, "in_s"), CC.frame(fx, "in_g"), device="cuda")
    CC.check_against_reference(out, fx)
