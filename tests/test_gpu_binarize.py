"""pert_rt_binarize (csrc/bin_kernels.hip) on the GPU: the kernel alone against the tensor program
on the same device, and the product path (kernel + host path for flagged cells) against the
reference's own outputs (tests/golden/binarize_reference.npz) and, at genome length, against the
per-cell sklearn restatement."""
import warnings

import numpy as np
import pytest
import torch

from scdna_replication_tools_amd import binarize as B
from tests import _bin_cases as C

pytestmark = pytest.mark.gpu
GENOME = (5451, 32, 7)            # bins, cells, seed of the genome-length case
CAPPED = ("A", "C", "genome")     # at most a tenth of these inputs' cells may be flagged


def _input(name):
    return C.simulated_ratio(*GENOME) if name == "genome" else C.matrix(name)


@pytest.fixture(scope="module")
def kernel_and_tensor():
    """Per input: the kernel's raw outputs and the tensor program's, both on the GPU, as numpy."""
    cache = {}

    def get(name):
        if name not in cache:
            X = torch.from_numpy(_input(name)).cuda()
            p = B.bin_params(X.shape[0])
            raw = {k: v.cpu().numpy() for k, v in B.native_binarize(X, p).items()}
            ten = {k: v.cpu().numpy() for k, v in B.tensor_binarize(X, p).items()}
            cache[name] = (X.cpu().numpy(), raw, ten)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def genome_reference():
    return C.sklearn_cells(_input("genome"))


@pytest.mark.parametrize("name", ["A", "B", "C", "E", "genome"])
def test_kernel_alone_matches_tensor_program(kernel_and_tensor, name):
    """Before any host path.  On every cell neither side flags: the same gmm_state, rt_state and
    chosen threshold; means, covariances and distances within the tolerance; n_rep the row sums
    of rt_state.  (The kernel has no k-means label output -- gmm_state's buffer is Lloyd's
    workspace until the final E step overwrites it -- so the k-means partition is checked through
    the EM it starts: another partition moves the means by far more than the tolerance.)"""
    X, raw, ten = kernel_and_tensor(name)
    ok = (raw["flags"] == 0) & (ten["flags"] == 0)
    print(name, "cells", ok.size, "kernel flags", int((raw["flags"] != 0).sum()), "tensor flags",
          int((ten["flags"] != 0).sum()))
    if name in CAPPED:
        assert (raw["flags"] != 0).mean() <= 0.10 and ok.mean() >= 0.90, (raw["flags"], ten["flags"])
    assert ok.any()
    np.testing.assert_array_equal(raw["gmm_state"][ok], ten["gmm_state"][ok])
    np.testing.assert_array_equal(raw["rt_state"][ok], ten["rt_state"][ok])
    np.testing.assert_array_equal(raw["best"][ok], ten["best"][ok])
    np.testing.assert_array_equal(raw["n_rep"], raw["rt_state"].sum(1))
    worst = {k: C.rel(raw[k][ok], ten[k][ok]) for k in ("means", "covs", "dist")}
    print(name, "worst relative differences", worst)
    assert max(worst.values()) <= C.RTOL, worst
    # the states are what the kernel's own threshold gives
    np.testing.assert_array_equal(raw["rt_state"], (X.T > np.linspace(-3, 3, 100)[raw["best"]][:, None]))
    assert set(np.unique(raw["gmm_state"])) <= {0, 1}


@pytest.mark.parametrize("case", C.CASES)
def test_product_path_matches_reference(case):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cn, man = B.binarize_profiles(C.table(case), "x", device="cuda")
    C.assert_profiles_are(case, cn, man)


@pytest.mark.parametrize("case", ["A", "B", "C", "E", "F"])
def test_matrix_product_path_matches_reference(case):
    g = C.golden()
    X = C.matrix(case)
    L, N = X.shape
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = B.binarize_matrix(torch.from_numpy(X).cuda())           # the tensor's device
    per_cell = lambda c: g["{}_{}".format(case, c)].reshape(N, L)
    np.testing.assert_array_equal(res.gmm_state.T, per_cell("gmm_state"))
    np.testing.assert_array_equal(res.rt_state.T, per_cell("rt_state"))
    np.testing.assert_array_equal(res.best_thresh, per_cell("binary_thresh")[:, 0])
    np.testing.assert_array_equal(res.frac_rt, per_cell("frac_rt")[:, 0])
    worst = dict(means=max(C.rel(res.means[:, j], per_cell("mean_%d" % j)[:, 0]) for j in (0, 1)),
                 covs=max(C.rel(res.covariances[:, j], per_cell("covariance_%d" % j)[:, 0]) for j in (0, 1)),
                 dist=C.rel(res.manhattan.reshape(-1), g[case + "_man_manhattan_dist"]))
    print(case, "flagged", int(res.flagged.sum()), "worst relative differences", worst)
    assert max(worst.values()) <= C.RTOL, worst


def test_genome_length_matches_sklearn_per_cell(genome_reference):
    X = _input("genome")
    ref = genome_reference
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = B.binarize_matrix(X, device="cuda")
    assert res.flagged.mean() <= 0.10, res.flags
    np.testing.assert_array_equal(res.gmm_state, ref["gmm_state"])
    np.testing.assert_array_equal(res.rt_state, ref["rt_state"])
    np.testing.assert_array_equal(res.best_thresh, np.linspace(-3, 3, 100)[ref["best"]])
    np.testing.assert_array_equal(res.frac_rt, ref["rt_state"].sum(0) / X.shape[0])
    worst = dict(means=C.rel(res.means, ref["means"]), covs=C.rel(res.covariances, ref["covariances"]),
                 dist=C.rel(res.manhattan, ref["manhattan"]))
    print("genome flagged", int(res.flagged.sum()), "worst relative differences", worst)
    assert max(worst.values()) <= C.RTOL, worst


def test_two_launches_are_bit_identical():
    X = torch.from_numpy(C.matrix("E")).cuda()
    p = B.bin_params(X.shape[0])
    a = {k: v.cpu().numpy() for k, v in B.native_binarize(X, p).items()}
    b = {k: v.cpu().numpy() for k, v in B.native_binarize(X, p).items()}
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_ragged_table_is_one_launch_per_length(monkeypatch):
    launches = []
    native = B.native_binarize

    def counting(X, p):
        launches.append(tuple(X.shape))
        return native(X, p)
    monkeypatch.setattr(B, "native_binarize", counting)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cn, man = B.binarize_profiles(C.table("D"), "x", device="cuda")
    assert sorted(launches) == [(263, 10), (271, 10), (300, 4)]
    cells = man["cell_id"].to_numpy()[::100]
    assert list(cells) == sorted(cells) and len(cells) == 24
    C.assert_profiles_are("D", cn, man)


def test_rejects_bad_arguments_on_the_device():
    import ctypes
    from scdna_replication_tools_amd import _native
    X = torch.from_numpy(C.matrix("C")).cuda()
    L, N = X.shape
    out = B.native_binarize(X, B.bin_params(L))
    ptrs = [out[k].data_ptr() for k in ("means", "covs", "gmm_state", "rt_state", "dist", "best", "n_rep", "flags")]
    p = B.bin_params(L)
    lib = _native.lib()
    assert lib.pert_rt_binarize(1, N, X.data_ptr(), ctypes.byref(p), *ptrs, None) == 1
    assert lib.pert_rt_binarize(L, N, None, ctypes.byref(p), *ptrs, None) == 1
    assert lib.pert_rt_binarize(L, N, X.data_ptr(), ctypes.byref(p), *ptrs[:7], None, None) == 1
    with pytest.raises(TypeError):
        B.binarize_matrix(X.float())
