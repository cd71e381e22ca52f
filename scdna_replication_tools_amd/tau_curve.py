"""Per-cell likelihood curves over S-phase time (tau) and the table read off them.

A fit reports one number for a cell's time in S phase, ``model_tau``.  ``PertShard.tau_curve``
evaluates, for every cell, the fit's objective along a grid of tau with everything else held at
the fit (pert_enum_evidence + pert_tau_curve); ``TauCurve`` holds the result and ``TauCurve.table``
turns it into a likelihood-ratio interval, a count of basins and the best alternative basin.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import pandas as pd

DEFAULT_GRID = np.linspace(0.01, 0.99, 99).astype(np.float32)
DEFAULT_DROP = 1.92            # half the 0.95 quantile of chi^2 with one degree of freedom

TABLE_COLUMNS = ["model_tau", "curve_at_fit", "curve_tau", "curve_gain", "tau_lo", "tau_hi", "n_modes", "alt_tau",
                 "alt_drop"]


def validate_grid(grid=None) -> np.ndarray:
    """The grid as a contiguous float32 vector: at least one and at most TAU_MAX_GRID finite values
    strictly inside (0, 1), strictly ascending (checked after the cast).  ``None`` is the default
    grid, np.linspace(0.01, 0.99, 99)."""
    from ._native import TAU_MAX_GRID
    if grid is None:
        return DEFAULT_GRID.copy()
    g = np.asarray(grid)
    if g.ndim != 1 or g.size < 1 or g.size > TAU_MAX_GRID:
        raise ValueError("the tau grid must be a vector of 1 to {} values".format(TAU_MAX_GRID))
    try:
        g = np.ascontiguousarray(g, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError("the tau grid must be numeric")
    if not np.isfinite(g).all():
        raise ValueError("the tau grid must be finite")
    if g.min() <= 0.0 or g.max() >= 1.0:
        raise ValueError("the tau grid must lie strictly inside (0, 1)")
    if g.size > 1 and not (np.diff(g) > 0).all():
        raise ValueError("the tau grid must be strictly ascending")
    return g


def u_prior_logpdf(u, mean_reads, ploidy, tau) -> np.ndarray:
    """log Normal(u_n ; g_n(tau), g_n(tau) / 10) with g_n(tau) = mean_reads_n / ((1 + tau) ploidy_n)
    (pert_model.py:597-600), fp64.  ``tau`` broadcasts against the per-cell vectors: (G, 1) gives
    (G, N).  NaN for a cell whose ploidy or mean read count is 0, where the model's prior is
    undefined."""
    u, mean_reads, ploidy = (np.asarray(v, np.float64) for v in (u, mean_reads, ploidy))
    with np.errstate(divide="ignore", invalid="ignore"):
        g = mean_reads / ((1.0 + np.asarray(tau, np.float64)) * ploidy)
        sd = g / 10.0
        return -0.5 * ((u - g) / sd) ** 2 - np.log(sd) - 0.5 * math.log(2.0 * math.pi)


class _Likelihood:
    """``TauCurve.likelihood_only``: the same quantities without the u-prior term."""

    def __init__(self, loglik: np.ndarray, at_fit: np.ndarray):
        self.loglik = loglik
        self.at_fit = at_fit


class TauCurve:
    """The fit's objective along tau, per cell, everything else at the fit.

    ``grid`` (G,) float32; ``loglik`` (G, N) float64, the sum over the bins of the element log
    marginals at tau = grid[g] plus the u prior's log density at that tau; ``at_fit`` (N,) the same
    at the cell's fitted tau; ``tau`` (N,) the fitted values; ``likelihood_only`` the same two
    arrays (``.loglik``, ``.at_fit``) without the u-prior term.

    This is a CONDITIONAL curve: pi, u, beta, rho and a stay at their fitted values and are not
    re-optimised per grid point (it is not a profile likelihood), so an interval read off it is a
    lower bound on tau's uncertainty.  The reads-only constant of the negative binomial is omitted
    as everywhere in the fit: only differences within a cell mean anything, not the level of a
    curve nor differences between cells.
    """

    def __init__(self, grid, loglik, at_fit, tau, likelihood_only: Optional[_Likelihood] = None):
        self.grid = np.asarray(grid, np.float32)
        self.loglik = np.asarray(loglik, np.float64)
        self.at_fit = np.asarray(at_fit, np.float64)
        self.tau = np.asarray(tau)
        if self.loglik.ndim != 2 or self.loglik.shape[0] != self.grid.size or self.grid.size < 1:
            raise ValueError("loglik must be (G, N) for a grid of G >= 1 values")
        if self.at_fit.shape != (self.loglik.shape[1],) or self.tau.shape != self.at_fit.shape:
            raise ValueError("at_fit and tau must be (N,)")
        self.likelihood_only = likelihood_only if likelihood_only is not None else _Likelihood(self.loglik, self.at_fit)

    @property
    def N(self) -> int:
        return self.loglik.shape[1]

    @property
    def G(self) -> int:
        return self.grid.size

    def table(self, drop: float = DEFAULT_DROP, cell_ids=None) -> pd.DataFrame:
        """One row per cell, computed in numpy fp64 from ``loglik`` (l_g) and ``at_fit`` (l(tau^)):

        * ``model_tau``, ``curve_at_fit``: the fitted tau and the curve's value there;
        * ``curve_tau``: the grid point of the highest value, the first on ties;
        * ``curve_gain`` = max_g l_g - l(tau^): how far the best grid point lies above the fit
          (negative when the fitted tau beats every grid point);
        * with l* = max(max_g l_g, l(tau^)) and S = {g : l_g >= l* - drop}: ``tau_lo`` / ``tau_hi``
          the least and greatest grid tau in S (NaN when S is empty), ``n_modes`` the number of
          maximal runs of consecutive grid indices in S;
        * ``alt_tau`` / ``alt_drop``: the best grid point (the first on ties) of the best run that
          does not hold ``curve_tau``, and l* minus its value (NaN when ``n_modes`` < 2).

        ``drop`` = 1.92 is half the 0.95 quantile of chi^2_1, the usual likelihood-ratio cut.  The
        curve is conditional -- pi, u, beta, rho and a stay at the fit -- so [tau_lo, tau_hi] is a
        lower bound on tau's uncertainty; and since the reads-only constant is omitted, only
        differences within a cell mean anything.  ``cell_ids`` becomes the first column ``cell_id``.
        """
        drop = float(drop)
        if not drop >= 0.0:
            raise ValueError("drop must be >= 0")
        ll, fit = self.loglik, self.at_fit
        G, N = ll.shape
        grid = self.grid.astype(np.float64)
        cols = np.arange(N)
        best = np.argmax(ll, axis=0)                               # first on ties
        top = ll[best, cols]
        star = np.maximum(top, fit)
        inS = ll >= (star - drop)[None, :]
        any_s = inS.any(axis=0)
        lo = np.where(any_s, grid[np.argmax(inS, axis=0)], np.nan)
        hi = np.where(any_s, grid[G - 1 - np.argmax(inS[::-1], axis=0)], np.nan)
        # a run starts where S holds and did not hold at the index before; its id counts the starts
        start = inS & ~np.vstack([np.zeros((1, N), bool), inS[:-1]])
        run_id = np.cumsum(start, axis=0)                          # 1-based inside S
        n_modes = start.sum(axis=0)
        alt = inS & (run_id != run_id[best, cols][None, :])        # S outside curve_tau's run
        masked = np.where(alt, ll, -np.inf)
        alt_i = np.argmax(masked, axis=0)
        has_alt = alt.any(axis=0)
        alt_tau = np.where(has_alt, grid[alt_i], np.nan)
        alt_drop = np.where(has_alt, star - np.where(has_alt, masked[alt_i, cols], 0.0), np.nan)
        out = pd.DataFrame({"model_tau": np.asarray(self.tau), "curve_at_fit": fit, "curve_tau": grid[best],
                            "curve_gain": top - fit, "tau_lo": lo, "tau_hi": hi, "n_modes": n_modes.astype(np.int64),
                            "alt_tau": alt_tau, "alt_drop": alt_drop}, columns=TABLE_COLUMNS)
        if cell_ids is not None:
            ids = np.asarray(cell_ids)
            if ids.shape != (N,):
                raise ValueError("cell_ids must name the curve's {} cells".format(N))
            out.insert(0, "cell_id", ids)
        return out
