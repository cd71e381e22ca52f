"""pert_boot_weights / pert_boot_counts / pert_boot_tfs_hist on the GPU: CellBootstrap's device path
and the C ABI against the host twins (integer counts: exact equality), at the smallest shapes
that cross each boundary of the kernels: N not a multiple of 16 and one past a 1024-cell chunk,
L one past a histogram tile and two tiles plus two, a launch boundary inside the replicates."""
import numpy as np
import pytest
import torch

from scdna_replication_tools_amd import cell_bootstrap as cb
from scdna_replication_tools_amd import rt_profiles as rt

pytestmark = pytest.mark.gpu

DTYPES = [(np.float32, np.float32), (np.float64, np.float64)]


@pytest.fixture(scope="module")
def nat():
    from scdna_replication_tools_amd import _native
    _native.lib()
    return _native


def labels(L, N, G):
    clone_ids = None
    if G > 1:                                                   # G - 1 clones and cells without one
        names = np.array(["k%02d" % g for g in range(G - 1)] + [None], object)
        clone_ids = names[(np.arange(N) * 11) % G]
    return dict(cell_ids=np.array(["c%04d" % ((7 * i) % N) for i in range(N)]),
                chr=np.array(["2", "10", "1"])[np.arange(L) % 3], start=np.arange(L)[::-1].copy(), clone_ids=clone_ids)


def matrices(L, N, G, seed=0):
    """(host RTMatrix, device RTMatrix on a strided tensor whose padding bytes are 0xFF)."""
    rng = np.random.default_rng(seed)
    rep = (rng.uniform(size=(L, N)) < 0.45).astype(np.uint8)
    ldn = -(-N // 16) * 16 + 16
    buf = torch.full((L, ldn), 0xFF, dtype=torch.uint8, device="cuda")
    buf[:, :N] = torch.from_numpy(rep).cuda()
    lab = labels(L, N, G)
    dev = rt.RTMatrix(buf[:, :N], **lab)
    assert dev._rep_dev.data_ptr() == buf.data_ptr() and dev.ldn == ldn            # used in place
    return rt.RTMatrix(rep, device="cpu", **lab), dev


def weights(B, N, seed=1):
    w = np.random.default_rng(seed).integers(0, 4, (B, N))
    w[0, 0], w[B - 1, N - 1], w[0, N // 2] = 255, 0, 0
    return w


def pad_weights_with_ff(boot):
    """The device copy of the weights with its padding columns set to 0xFF: they must never count."""
    w = torch.full((boot.n_boot, boot.ldw), 0xFF, dtype=torch.uint8, device="cuda")
    w[:, :boot.N] = torch.from_numpy(boot.weights).cuda()
    boot._w_dev = w


def assert_same(dev, host, G):
    for a, b in zip(dev.counts('clone'), host.counts('clone')):
        assert a.dtype == np.int64 and a.shape == b.shape and (a == b).all()
    for dtype, frac_dtype in DTYPES:
        for by in (('population', 'clone') if G > 1 else ('population',)):
            got = dev.tfs_counts(by=by, dtype=dtype, frac_dtype=frac_dtype)
            want = host.tfs_counts(by=by, dtype=dtype, frac_dtype=frac_dtype)
            for a, b in zip(got, want):
                assert a.dtype == np.int64 and a.shape == b.shape and (a == b).all(), (by, dtype)
            assert want[0].sum() > 0


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("L,N", [(65, 37), (130, 1030)])
def test_explicit_weights_match_the_host_twin(L, N, G, B):
    host_m, dev_m = matrices(L, N, G)
    w = weights(B, N)
    host = cb.CellBootstrap(host_m, weights=w)
    dev = cb.CellBootstrap(dev_m, weights=w, chunk=2)           # B = 5: launches of 2, 2 and 1 replicates
    pad_weights_with_ff(dev)
    assert_same(dev, host, G)


def test_counts_abi_masks_both_operands(nat):
    L, N, C = 65, 1030, 11                                      # C: a second, partial tile of weight rows
    host_m, dev_m = matrices(L, N, 1)
    rng = np.random.default_rng(5)
    ldw = 1040
    wg = np.full((C, ldw), 0xFF, np.uint8)
    wg[:, :N] = rng.integers(0, 256, (C, N))
    wg[3, :N] = 0
    wg_d = torch.from_numpy(wg).cuda()
    out = []
    for _ in range(2):
        count = torch.zeros((C, L), dtype=torch.int32, device="cuda")
        nat.check(nat.lib().pert_boot_counts(L, N, dev_m.ldn, dev_m._rep_dev.data_ptr(), C, ldw, wg_d.data_ptr(),
                                             count.data_ptr(), torch.cuda.current_stream().cuda_stream),
                  "pert_boot_counts")
        out.append(count.cpu().numpy().view(np.uint32).astype(np.int64))
    want = wg[:, :N].astype(np.int64) @ host_m._rep_host.astype(np.int64).T
    assert (out[0] == want).all() and (out[1] == want).all() and not out[0][3].any()


def test_weights_kernel_is_the_host_resampler(nat):
    N = 1030
    strata = np.full(N, 2)
    strata[[5, 100, 333, 640, 1000, 1029]] = 1                  # strata of 1, 6 and 1023 cells
    strata[517] = 0
    order, pos_lo, pos_n = cb.stratum_layout(strata)
    seed, b0, B, ldw = (3 << 40) + 17, (1 << 32) + 2, 5, 1040
    tensors = [torch.as_tensor(a, device="cuda") for a in (pos_lo, pos_n, order)]
    out = []
    for _ in range(2):
        scratch = torch.zeros((B, N), dtype=torch.int32, device="cuda")
        w = torch.full((B, ldw), 0xEE, dtype=torch.uint8, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        nat.check(nat.lib().pert_boot_weights(N, ldw, *(t.data_ptr() for t in tensors), seed, b0, B,
                                              scratch.data_ptr(), w.data_ptr(), flag.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "pert_boot_weights")
        assert int(flag.item()) == 0
        out.append(w.cpu().numpy())
    assert (out[0] == out[1]).all() and not out[0][:, N:].any()
    want = cb.boot_weights_host(strata, B, seed=seed, b0=b0)
    assert (out[0][:, :N] == want).all()
    assert (want[:, 517] == 1).all() and (want[:, strata == 1].sum(axis=1) == 6).all()


def test_generated_weights_reruns_and_chunking():
    L, N, G, B = 65, 1030, 4, 5
    host_m, dev_m = matrices(L, N, G)
    host = host_m.bootstrap(n_boot=B, seed=9)
    first = dev_m.bootstrap(n_boot=B, seed=9)
    assert first.weights.dtype == np.uint8 and (first.weights == host.weights).all()
    assert_same(first, host, G)
    ref = first.counts('clone') + first.tfs_counts(by='clone')
    for chunk in (None, 1, 2, B):                               # None: the run again, as it was
        again = dev_m.bootstrap(n_boot=B, seed=9, chunk=chunk)
        assert again.weights.tobytes() == first.weights.tobytes()
        for a, b in zip(ref, again.counts('clone') + again.tfs_counts(by='clone')):
            assert a.tobytes() == b.tobytes(), chunk


def test_more_groups_than_one_launch_holds(nat):
    L, N, G = 65, 1030, nat.RT_MAX_GROUPS + 3                   # by='clone': 34 groups, two launches per chunk
    host_m, dev_m = matrices(L, N, G)
    w = weights(2, N)
    assert_same(cb.CellBootstrap(dev_m, weights=w), cb.CellBootstrap(host_m, weights=w), G)


def test_refusals_write_nothing(nat):
    L, N, B = 65, 37, 2
    _, dev_m = matrices(L, N, 1)
    ldw = 48
    w = torch.ones((B, ldw), dtype=torch.uint8, device="cuda")
    grp = torch.zeros(N, dtype=torch.int32, device="cuda")
    f10 = torch.zeros(N, dtype=torch.float32, device="cuda")
    edges = torch.linspace(-10, 10, nat.RT_MAX_EDGES + 1, dtype=torch.float32, device="cuda")
    hours = torch.zeros((B, nat.RT_MAX_GROUPS + 1, L), dtype=torch.float32, device="cuda")
    hn = torch.zeros((B, nat.RT_MAX_GROUPS + 1, nat.RT_MAX_EDGES), dtype=torch.int32, device="cuda")
    hr = torch.zeros_like(hn)

    def call(G, n_edges):
        return nat.lib().pert_boot_tfs_hist(L, N, dev_m.ldn, G, dev_m._rep_dev.data_ptr(), grp.data_ptr(), B, ldw,
                                            w.data_ptr(), hours.data_ptr(), f10.data_ptr(), edges.data_ptr(), n_edges,
                                            0, hn.data_ptr(), hr.data_ptr(), torch.cuda.current_stream().cuda_stream)

    assert call(nat.RT_MAX_GROUPS + 1, 201) == 1                # PERT_E_ARG, before any launch
    assert call(1, nat.RT_MAX_EDGES + 1) == 1
    torch.cuda.synchronize()
    assert not hn.any() and not hr.any()
    assert call(nat.RT_MAX_GROUPS, nat.RT_MAX_EDGES) == 0       # the largest accepted call runs
    torch.cuda.synchronize()
    assert int(hn.sum()) == B * L * N


def test_unit_weights_reproduce_the_matrix():
    L, N, G = 130, 1030, 4
    _, dev_m = matrices(L, N, G)
    boot = cb.CellBootstrap(dev_m, weights=np.ones((2, N), np.uint8))
    count, size = boot.counts('clone')
    clone_count, _ = dev_m.counts()
    assert (count[0] == clone_count).all() and (count[1] == clone_count).all()
    assert (size[0] == np.bincount(boot._group, minlength=G)).all()
    for dtype, frac_dtype in DTYPES:
        kw = dict(dtype=dtype, frac_dtype=frac_dtype)
        pop = boot.tfs_counts(by='population', **kw)
        clone = boot.tfs_counts(by='clone', **kw)
        for i in range(2):
            assert (pop[i][1, 0] == dev_m.tfs_counts(by='population', **kw)[i]).all()
            assert (clone[i][1].sum(axis=0) == dev_m.tfs_counts(by='clone', **kw)[i]).all()
