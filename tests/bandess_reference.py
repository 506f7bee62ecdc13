"""An independent numpy statement of the band ESS mode's definition (include/tamcmc_accel.h, "ESS AND MCSE OF THE
CREDIBLE-BAND EDGES"), for tests/test_summary_bandess_gpu.py and tests/test_cli_bandess_gpu.py, and what those suites share.
Nothing here is shared with the library.

counts()      b = rows <= thr, then N, C_k, H_k, T_k as integer sums and E_k in Python ints (no width to overflow), for
              k = 0 ... L.  None of them depends on L beyond the range of k: a larger L extends the arrays.
reference()   the whole result of one pass for K thresholds at lag limit L: the counts, ess_reference.finish on
              E.astype(float64), p_hat, mcse_p and the totals.
"""
import numpy as np

import ess_reference as R
from support import bits

ARRAYS = ("count_le", "p_hat", "ess", "tau", "mcse_p", "cut")
TOTALS = ("n_used", "n_rejected", "lag", "n_thresholds", "min_ess", "bin_min_ess", "n_truncated", "n_constant")


def counts(rows, thr, L):
    """rows (n, Nx) of the accepted samples, thr (Nx,).  Returns N (Nx,) int64, C (L + 1, Nx) int64 and E (L + 1, Nx) of
    Python ints."""
    with np.errstate(invalid="ignore"):
        b = (np.asarray(rows) <= np.asarray(thr)[None, :]).astype(np.int64)
    n, nx = b.shape
    N = b.sum(axis=0)
    C, H, T = (np.zeros((L + 1, nx), dtype=np.int64) for _ in range(3))
    for k in range(L + 1):
        C[k] = (b[k:] * b[:n - k]).sum(axis=0)
        H[k] = b[:k].sum(axis=0)
        T[k] = b[n - k:].sum(axis=0) if k else 0
    No, Co, Ho, To = (a.astype(object) for a in (N, C, H, T))
    k = np.arange(L + 1).astype(object)[:, None]
    E = n * n * Co - n * No * (2 * No - Ho - To) + (n - k) * No * No
    assert all(int(E[0, i]) == n * int(N[i]) * (n - int(N[i])) for i in range(nx))
    return N, C, E


def finish(E, n, L):
    """tau, ess, cut of ess_reference.finish on the first L + 1 rows of E, converted to float64 (one rounding each)."""
    return R.finish(np.asarray(E[:L + 1]).astype(np.float64), n)


def first_min(v):
    """(min, bin) with the first bin winning a tie and a NaN skipped; (NaN, -1) if every value is NaN."""
    v = np.asarray(v, dtype=np.float64)
    if np.all(np.isnan(v)):
        return np.nan, -1
    k = int(np.argmin(np.where(np.isnan(v), np.inf, v)))
    return v[k], k


class Counts:
    """The counts of one chain for a list of thresholds, computed once at the largest lag limit any test of the chain uses."""

    def __init__(self, rows, thr, Lmax):
        self.rows, self.thr, self.n = rows, np.atleast_2d(thr), len(rows)
        self.per = [counts(rows, t, Lmax) for t in self.thr]
        self._fin = {}

    def finish(self, j, L):
        if (j, L) not in self._fin:
            self._fin[(j, L)] = finish(self.per[j][2], self.n, L)
        return self._fin[(j, L)]


def ulps(a, b):
    """max |a - b| in ulps of b; NaN must meet NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    if not ok.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        d = np.where(a[ok] == b[ok], 0.0, np.abs(a[ok] - b[ok]) / np.spacing(np.abs(b[ok])))
    return float(np.max(d))


WORST = {"tau": 0.0, "ess": 0.0}


def check_exact(tag, res, ref, L, n_rejected=0):
    """Case 1 of the GPU suite: `res` (run_band's dict: bandess_result plus "C" and "E", lists over the thresholds) against
    the Counts `ref`, whose first K thresholds are the ones the pass was given."""
    K, n = res["n_thresholds"], ref.n
    assert res["n_used"] == n and res["n_rejected"] == n_rejected and res["lag"] == L and K == len(res["C"]), tag
    worst = {"tau": 0.0, "ess": 0.0}
    for j in range(K):
        N, C, E = ref.per[j]
        assert res["C"][j].dtype == np.int32 and res["E"][j].dtype == np.int64
        assert np.array_equal(res["C"][j], C[:L + 1]), (tag, j, "C_k")
        assert np.array_equal(res["E"][j].astype(object), E[:L + 1]), (tag, j, "E_k")
        assert np.array_equal(res["count_le"][j], N), (tag, j, "count_le")
        tau, ess, cut = ref.finish(j, L)
        assert np.array_equal(res["cut"][j], cut), (tag, j, "cut")
        worst["tau"] = max(worst["tau"], ulps(res["tau"][j], tau))
        worst["ess"] = max(worst["ess"], ulps(res["ess"][j], ess))
        p = N.astype(np.float64) / np.float64(n)
        assert np.array_equal(bits(res["p_hat"][j]), bits(p)), (tag, j, "p_hat")
        with np.errstate(invalid="ignore", divide="ignore"):
            m = np.sqrt(p * (1.0 - p) / res["ess"][j])
        assert np.array_equal(bits(res["mcse_p"][j]), bits(m)), (tag, j, "mcse_p")
        const = (N == 0) | (N == n)
        assert np.all(np.isnan(res["ess"][j][const])) and np.all(np.isnan(res["tau"][j][const])) and np.all(res["cut"][j][const] == 0), (tag, j)
        assert np.all(np.isfinite(res["ess"][j][~const])), (tag, j)
        v, k = first_min(res["ess"][j])
        assert bits(res["min_ess"][j]) == bits(v) and res["bin_min_ess"][j] == k, (tag, j, "min_ess")
        assert res["n_truncated"][j] == int((res["cut"][j] == L + 1).sum()) and res["n_constant"][j] == int(const.sum()), (tag, j)
    print(f"ULPS bandess {tag} L={L} K={K}: " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    for k, v in worst.items():
        WORST[k] = max(WORST[k], v)
        assert v <= 4.0, (tag, k, v)


def same_band(r1, r2, skip=()):
    """Two results of run_band bit for bit: every array, every total, and the counts where both have them."""
    for k in ARRAYS + TOTALS:
        if k in skip:
            continue
        a, b = np.asarray(r1[k], dtype=np.float64), np.asarray(r2[k], dtype=np.float64)
        if a.shape != b.shape or not np.array_equal(bits(a), bits(b)):
            return False
    for k in ("C", "E"):
        if k in r1 and k in r2:
            if len(r1[k]) != len(r2[k]) or not all(np.array_equal(a, b) for a, b in zip(r1[k], r2[k])):
                return False
    return True
