"""chainsummary_hip --loo-window on the GPU: the 23-sample chain of summary_support.stored_chain on the golden local-model
inputs.  <output file>.loowin parses -- the totals in its header, one row per window -- and holds the numbers
Summary.window_loo(rows, W, first, pit=...) gives, to the 12 printed digits; with --loo-pit the five PIT columns and their
totals are there as well; the main output file is, byte for byte, what the same binary writes without the option, and without
it no .loowin file appears."""
import os
import subprocess

import numpy as np
import pytest

from summary_support import f12, header_values, stored_chain
from tamcmc_amd import capi

pytestmark = pytest.mark.gpu

COLUMNS = ("first_bin", "last_bin", "x_first", "x_last", "elpd_lwo", "pareto_k", "tail_len")
PIT_COLUMNS = ("loo_pit", "loo_log_cdf", "loo_log_sf", "is_ess", "log_wsum")


def test_command_line(accel_mod, tmp_path):
    s, root, v, rows, common, sel = stored_chain(tmp_path)
    W, first = 20, 7
    with accel_mod.Accel(s.model_case, s.plength, s.x, s.y, sigma_y=s.sigma_y, likelihood_case=s.likelihood_case,
                         likelihood_p=s.likelihood_p) as acc:
        with capi.Summary(acc) as sm:
            _, st = sm.push(rows)
            d = sm.window_loo(rows, W, first, pit=True)
            d0 = sm.window_loo(rows, W)
    assert np.all(st == 0) and d["n_used"] == 23 and d["n_rejected"] == 0
    x = np.asarray(s.x)
    for tag, flags, want, pit in (("a", ["--loo-window", "%d,%d" % (W, first)], d, False), ("b", ["--loo-window", "%d,%d" % (W, first), "--loo-pit"], d, True),
                                  ("c", ["--loo-window", str(W)], d0, False)):
        base = ["--loo-pit"] if pit else []
        plain, table = str(tmp_path / (tag + "_plain.txt")), str(tmp_path / (tag + ".txt"))
        r = subprocess.run(common + [plain] + sel + base, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert not os.path.exists(plain + ".loowin")
        r = subprocess.run(common + [table] + sel + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert open(table, "rb").read().replace(table.encode(), b"@") == open(plain, "rb").read().replace(plain.encode(), b"@"), \
            "the output file is not that of a run without --loo-window"
        if pit:
            assert open(table + ".loopit", "rb").read() == open(plain + ".loopit", "rb").read()
        lines = open(table + ".loowin").read().split("\n")
        head = header_values(line for line in lines if line.startswith("#") and "=" in line)
        nhead = 7 if pit else 4
        assert lines[0].startswith("# chainsummary_hip (") and lines[nhead] == "# " + " ".join(COLUMNS + (PIT_COLUMNS if pit else ()))
        for k in ("W", "first", "n_windows", "n_used", "n_rejected", "n_k_high", "n_k_inf"):
            assert int(head[k]) == want[k], k
        for k, name in (("elpd_lwo", "elpd_lwo_total"), ("p_lwo", "p_lwo"), ("k_max", "k_max")):
            assert head[k] == "%.12g" % want[name], k
        if pit:
            for k, name in (("win_min_log_sf", "bin_min_loo_log_sf"), ("win_min_log_cdf", "bin_min_loo_log_cdf"), ("win_min_is_ess", "bin_min_is_ess")):
                assert int(head[k]) == want[name], k
            for k, name in (("ks_D", "loo_ks_D"), ("min_log_sf", "min_loo_log_sf"), ("min_log_cdf", "min_loo_log_cdf"), ("min_is_ess", "min_is_ess")):
                assert head[k] == "%.12g" % want[name], k
            assert [int(t) for t in lines[6].split("=")[1].split()] == list(want["loo_pit_hist"]) and sum(want["loo_pit_hist"]) == want["n_windows"]
        t = np.loadtxt(table + ".loowin", ndmin=2)
        assert t.shape == (want["n_windows"], len(COLUMNS) + (len(PIT_COLUMNS) if pit else 0))
        assert np.array_equal(t[:, 0], want["first_bin"]) and np.array_equal(t[:, 1], want["last_bin"])
        assert np.array_equal(t[:, 2], f12(x[want["first_bin"]])) and np.array_equal(t[:, 3], f12(x[want["last_bin"]]))
        assert np.array_equal(t[:, 4], f12(want["elpd_lwo"])) and np.array_equal(t[:, 5], f12(want["pareto_k"]), equal_nan=True)
        assert np.array_equal(t[:, 6], want["tail_len"])
        for j, k in enumerate(PIT_COLUMNS if pit else (), start=len(COLUMNS)):
            assert np.array_equal(t[:, j], f12(want[k]), equal_nan=True), k
