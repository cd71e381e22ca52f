"""Independent numpy side of the simulator tests: a Philox4x32-10 written from the paper
(Salmon et al., SC'11), the counter rule and uniform mapping that include/pert_hip.h documents,
and the distribution statistics with their derived thresholds."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
TAG_CELLS, TAG_READS = 1, 2
MASK = np.uint64(0xFFFFFFFF)


def philox(counter, key):
    """counter: uint32 [..., 4]; key: (k0, k1).  Returns uint32 [..., 4]."""
    c = [np.asarray(counter[..., i], np.uint64) for i in range(4)]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def make_key(seed, tag):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, (seed >> 32) ^ ((tag * 0x9E3779B9) & 0xFFFFFFFF)


def draw(seed, tag, bins, cells, rnd):
    """Words of (bin, global cell, draw round), broadcast over bins and cells: uint32 [..., 4]."""
    bins, cells = np.broadcast_arrays(np.asarray(bins, np.uint64), np.asarray(cells, np.uint64))
    ctr = np.stack([bins & MASK, cells & MASK, np.full(bins.shape, rnd, np.uint64), cells >> np.uint64(32)], axis=-1)
    return philox(ctr, make_key(seed, tag))


def uniform64(w):
    """((w >> 8) + 0.5) 2^-24, exact in float64."""
    return ((np.asarray(w, np.uint32) >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def uniform32(w):
    """The documented fp32 uniform: rounded once, the value that rounds to 1 kept below it."""
    return np.minimum(uniform64(w).astype(np.float32), np.float32(1.0 - 2.0 ** -24))


def cell_draws(seed, cell0, libs, beta_means, beta_stds):
    """tau float32 [N] and betas float32 [K1][N] of the documented per-cell rule, Box-Muller in float64."""
    libs = np.asarray(libs)
    cells = cell0 + np.arange(len(libs))
    tau = uniform32(draw(seed, TAG_CELLS, 0, cells, 0)[:, 0])
    K1 = beta_means.shape[1]
    betas = np.empty((K1, len(libs)), np.float32)
    for k in range(K1):
        w = draw(seed, TAG_CELLS, 0, cells, 1 + k)
        z = np.sqrt(-2.0 * np.log(uniform64(w[:, 0]))) * np.cos(2.0 * np.pi * uniform64(w[:, 1]))
        betas[k] = (beta_means[libs, k].astype(np.float64) + beta_stds[libs, k].astype(np.float64) * z
                    ).astype(np.float32)
    return tau, betas


# ---------------------------------------------------------------- negative-binomial statistics

def nb_moments(delta, lamb):
    """Mean, variance and fourth central moment of NegativeBinomial(delta, probs=lamb) (torch's
    parametrisation: lamb is the success probability of the counted events), elementwise."""
    delta = np.asarray(delta, np.float64)
    q = 1.0 - lamb
    mean = delta * lamb / q
    var = delta * lamb / q ** 2
    # excess kurtosis 6 / delta + q^2 / (lamb delta)
    m4 = var ** 2 * (3.0 + 6.0 / delta + q ** 2 / (lamb * delta))
    return mean, var, m4


def nb_chi2(sample, delta, lamb, max_bins=34, min_expected=20.0):
    """Pearson chi-square of ``sample`` against scipy's nbinom(delta, 1 - lamb): at most
    ``max_bins`` bins between the 0.1 % and 99.9 % quantiles (the two tails are the outer bins),
    neighbours merged until every expected count is at least ``min_expected``.
    Returns (statistic, degrees of freedom, smallest expected count)."""
    from scipy import stats
    dist = stats.nbinom(delta, 1.0 - lamb)
    n = sample.size
    lo, hi = int(dist.ppf(0.001)), int(dist.ppf(0.999))
    width = max(1, -(-(hi - lo + 1) // (max_bins - 2)))
    inner = np.arange(lo, hi + 1, width)                     # left ends of the inner bins
    # bin b holds the integers in [edges[b], edges[b + 1])
    edges = np.concatenate([[0], inner, [hi + 1]]) if lo > 0 else np.concatenate([inner, [hi + 1]])
    edges = np.unique(edges)
    cdf = np.concatenate([[0.0], dist.cdf(edges[1:] - 1), [1.0]])
    expected = list(np.diff(cdf) * n)                        # the last bin is [hi + 1, inf)
    observed = list(np.histogram(sample, bins=np.concatenate([edges, [np.inf]]))[0].astype(np.float64))
    i = 0
    while i < len(expected):                                 # merge forwards, the tail backwards
        if expected[i] < min_expected and len(expected) > 1:
            j = i + 1 if i + 1 < len(expected) else i - 1
            expected[j] += expected[i]
            observed[j] += observed[i]
            del expected[i], observed[i]
            i = max(i - 1, 0) if j < i else i
        else:
            i += 1
    expected, observed = np.asarray(expected), np.asarray(observed)
    assert len(expected) <= max_bins and abs(expected.sum() - n) < 1e-6 * n and observed.sum() == n
    stat = float(((observed - expected) ** 2 / expected).sum())
    return stat, len(expected) - 1, float(expected.min())


def chi2_threshold(df, alpha=1e-6):
    from scipy import stats
    return float(stats.chi2.ppf(1.0 - alpha, df))
