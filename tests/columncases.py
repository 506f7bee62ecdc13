"""Columns of extreme values for the mode table's column kernels (tests/test_mode_columns_gpu.py), their host checks
(tests/test_columncases_host.py) and the layouts they are planted in.  Every set is a deterministic function of its name and
n.  Importing this module needs no GPU.

  zeros        alt: +0, -0 alternating; among: +-0 between normal values of both signs.
  denormals    +-5e-324, +-1e-323, +-DBL_MIN and its two neighbours, +-0.  smallest: 0, +-5e-324, +-1e-323 only, so that
               hi - lo <= 3e-323 and the histogram scale n_bins / (hi - lo) overflows for every n_bins.
  span64       -DBL_MAX ... +DBL_MAX, a decade apart, both signs; inf: -inf and +inf at the ends.  Either way
               bit_length(key(max) - key(min)) = 64: eight 8-bit digits in the table's quantile kernel, u >= 64 in tmq_match.
  neighbours   3 ... 300 consecutive doubles (a nextafter chain) around 110.2, each about n / m times: the keys differ in their
               last bits only, the histogram classes are decided by single ulps of (v - lo) * s.
  infs         finite values with one +inf (plus), one -inf (minus) or both (both).
  huge         finite values of magnitude 1e300, both signs: the Welford M2, the lag products and the covariance overflow.
  ties         equal: all equal; but_one: all equal but one; halves: two values half and half; twice: every value twice.
  scaled       span64's finite values times 2^-600: the same eight digits with no overflow in any sum.

plant(w, values) puts a column into the frequency of an l = 0 mode of a local layout: the freq column equals the params entry
bit for bit, nu_m repeats it, and the truncation window clamps a mode outside the grid, so every non-NaN double is a row of
status 0."""
import math

import numpy as np

from tamcmc_amd import synth

DBL_MAX, DBL_MIN, DENORM = np.finfo(np.float64).max, np.finfo(np.float64).tiny, 5e-324
SIZES = (1, 2, 64, 257, 4097, 8193)
SETS = ("zeros-alt", "zeros-among", "denormals", "denormals-smallest", "span64", "span64-inf", "neighbours", "infs-plus", "infs-minus",
        "infs-both", "huge", "ties-equal", "ties-but_one", "ties-halves", "ties-twice", "scaled")
MIN_N = {"span64": 2, "span64-inf": 2, "neighbours": 3, "infs-plus": 2, "infs-minus": 2, "infs-both": 3, "huge": 2, "ties-but_one": 2,
         "ties-halves": 2, "ties-twice": 2, "scaled": 2, "zeros-among": 2}
FREQ_COL, NU_COL = 4, 11                 # the single mode's freq and nu_m columns of the 13-column layout


def _shuffled(v, seed):
    return np.asarray(v, dtype=np.float64)[np.random.default_rng(seed).permutation(len(v))]


def _decades(n):
    """n values from -DBL_MAX to +DBL_MAX: +-10^e a decade apart around zero, the ends exact."""
    half = n // 2
    e = np.linspace(-300.0, 300.0, max(half, 1))
    pos = 10.0 ** np.round(e)
    v = np.concatenate([-pos[::-1][:half], [0.0] * (n - 2 * half), pos[:half]])
    v = np.sort(v)
    v[0], v[-1] = -DBL_MAX, DBL_MAX
    return v


def column(name, n, seed=0):
    """The n values of set `name` in push order (float64)."""
    assert name in SETS and n >= MIN_N.get(name, 1), (name, n)
    i = np.arange(n)
    if name == "zeros-alt":
        return np.where(i % 2 == 0, 0.0, -0.0)
    if name == "zeros-among":
        v = _shuffled(np.linspace(-3.0, 3.0, n) + 0.015625, seed + 1)
        v[i % 3 == 0] = 0.0
        v[i % 6 == 3] = -0.0
        return v
    if name in ("denormals", "denormals-smallest"):
        small = [0.0, -0.0, DENORM, -DENORM, 2 * DENORM, -2 * DENORM]
        edge = [DBL_MIN, -DBL_MIN, np.nextafter(DBL_MIN, 0.0), -np.nextafter(DBL_MIN, 0.0), np.nextafter(DBL_MIN, 1.0),
                -np.nextafter(DBL_MIN, 1.0)]
        pool = np.array(small if name.endswith("smallest") else small + edge)
        return _shuffled(pool[i % pool.size], seed + 2)
    if name in ("span64", "span64-inf", "scaled"):
        v = _decades(n)
        if name == "span64-inf":
            v[0], v[-1] = -np.inf, np.inf
        if name == "scaled":
            v = v * 2.0 ** -600
        return _shuffled(v, seed + 3)
    if name == "neighbours":
        m = min(n, 300)
        chain = np.empty(m)
        chain[0] = 110.2
        for k in range(1, m):
            chain[k] = np.nextafter(chain[k - 1], np.inf)
        chain = chain[np.argsort(np.abs(np.arange(m) - m // 3), kind="stable")]      # 110.2 is neither end of the chain's use
        return _shuffled(np.sort(chain)[i % m], seed + 4)
    if name.startswith("infs"):
        v = _shuffled(100.0 + 0.25 * i, seed + 5)
        if name in ("infs-plus", "infs-both"):
            v[n // 3] = np.inf
        if name in ("infs-minus", "infs-both"):
            v[(2 * n) // 3 if name == "infs-both" else n // 3] = -np.inf
        return v
    if name == "huge":
        return _shuffled(np.where(i % 2 == 0, 1.0, -1.0) * 1e300 * (1.0 + (i % 7) * 0.125), seed + 6)
    if name == "ties-equal":
        return np.full(n, 110.2)
    if name == "ties-but_one":
        v = np.full(n, 110.2)
        v[n // 2] = 110.25
        return v
    if name == "ties-halves":
        return _shuffled(np.where(i < n // 2, 110.25, 110.2), seed + 7)
    assert name == "ties-twice"
    return _shuffled(110.0 + 0.5 * (i // 2), seed + 8)


def sizes(name):
    return [n for n in SIZES if n >= MIN_N.get(name, 1)]


def one_mode():
    """id 11 (local) with a single l = 0 mode: 13 columns (the layout of the rank and pdf suites)."""
    Nx = 1500
    x = synth.grid(Nx, 94.30, 40.0 / Nx)
    p = np.array([12.0, 110.2, 0.4, 0.0, 0.0, math.sqrt(0.4) * 0.5, math.sqrt(0.4) * math.sqrt(0.75), 0.0, 0.15, 0.8, 60.0, 20.0, 0.0])
    pl = np.array([1, 0, 1, 0, 0, 0, 6, 1, 1, 1, 2], dtype=np.int32)
    return dict(model_case=11, plength=pl, params_true=p, x=x, freq_index=[1], freq_cols=[4], nu_cols=[11])


def two_modes():
    """id 11 with two l = 0 modes: 22 columns, two columns to plant (pairs, covariance, correlation)."""
    Nx = 1500
    x = synth.grid(Nx, 94.30, 40.0 / Nx)
    p = np.array([12.0, 9.0, 110.2, 125.7, 0.4, 0.0, 0.0, math.sqrt(0.4) * 0.5, math.sqrt(0.4) * math.sqrt(0.75), 0.0, 0.15, 0.18, 0.8, 60.0,
                  20.0, 0.0])
    pl = np.array([2, 0, 2, 0, 0, 0, 6, 2, 1, 1, 2], dtype=np.int32)
    return dict(model_case=11, plength=pl, params_true=p, x=x, freq_index=[2, 3], freq_cols=[4, 13], nu_cols=[11, 20])


def plant(w, *columns):
    """Params rows of workload w whose k-th l = 0 frequency is columns[k]; every other entry is params_true's."""
    n = len(columns[0])
    P = np.tile(w["params_true"], (n, 1))
    for idx, v in zip(w["freq_index"], columns):
        assert len(v) == n and not np.any(np.isnan(v))
        P[:, idx] = v
    return P


def expected_rows(w, base_row, *columns):
    """The table rows plant() must give: base_row (the derived row of params_true) with the planted values in the freq and nu_m
    columns.  The window columns are checked apart (they follow the frequency)."""
    n = len(columns[0])
    rows = np.tile(np.asarray(base_row, dtype=np.float64), (n, 1))
    for fc, nc, v in zip(w["freq_cols"], w["nu_cols"], columns):
        rows[:, fc] = v
        rows[:, nc] = v
    return rows
