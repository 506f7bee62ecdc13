"""bin/chainsummary_hip --window on the GPU: the 23-sample chain of summary_support.stored_chain on the golden
local-model inputs.  --window 7,3 writes <output file>.windows, whose header and rows are the numbers
Summary(..., window=(7, 3)).window_result() gives to the 12 printed digits; the output file itself is, byte for byte, what
the same binary writes without the flag, with and without --predictive."""
import os
import subprocess

import numpy as np
import pytest

from summary_support import f12, header_values, stored_chain
from tamcmc_amd import capi

pytestmark = pytest.mark.gpu


def test_command_line(accel_mod, tmp_path):
    s, root, v, rows, common, sel = stored_chain(tmp_path)
    with accel_mod.Accel(s.model_case, s.plength, s.x, s.y, sigma_y=s.sigma_y, likelihood_case=s.likelihood_case,
                         likelihood_p=s.likelihood_p) as acc:
        with capi.Summary(acc, window=(7, 3)) as sm:
            _, st = sm.push(rows)
            d = sm.window_result()
    assert np.all(st == 0) and d["n_used"] == 23 and d["n_windows"] == 1 + -(-(s.Nx - 3) // 7)
    for extra in ([], ["--predictive"]):
        plain, table = str(tmp_path / f"plain{len(extra)}.txt"), str(tmp_path / f"win{len(extra)}.txt")
        for path, flag in ((plain, []), (table, ["--window", "7,3"])):
            r = subprocess.run(common + [path] + sel + extra + flag, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout + r.stderr
        assert open(table, "rb").read() == open(plain, "rb").read(), "the output file changed with --window"
        assert not os.path.exists(plain + ".windows")
        lines = open(table + ".windows").read().split("\n")
        head = [line for line in lines if line.startswith("#")]
        assert lines[:len(head)] == head and lines[-1] == "" and len(lines) == len(head) + d["n_windows"] + 1
        assert head[0].startswith("# chainsummary_hip (") and head[-1] == "# w first_bin last_bin x_first x_last pit log_cdf log_sf mean_resid"
        val = header_values(head[1:-2])
        for key in ("W", "first", "n_windows", "n_used", "n_rejected", "win_min_log_sf", "win_min_log_cdf"):
            assert int(val[key]) == d[key], key
        assert (d["W"], d["first"]) == (7, 3)
        for key in ("ks_D", "min_log_sf", "min_log_cdf"):
            assert val[key] == "%.12g" % d[key], key
        assert head[-2].startswith("# pit_hist=")
        hist = [int(c) for c in head[-2].split("=")[1].split()]
        assert hist == list(d["pit_hist"]) and sum(hist) == d["n_windows"]
        t = np.loadtxt(table + ".windows")
        assert t.shape == (d["n_windows"], 9)
        assert np.array_equal(t[:, 0], np.arange(d["n_windows"])) and np.array_equal(t[:, 1], d["first_bin"]) and np.array_equal(t[:, 2], d["last_bin"])
        assert np.array_equal(t[:, 3], f12(s.x[d["first_bin"]])) and np.array_equal(t[:, 4], f12(s.x[d["last_bin"]]))
        for j, key in enumerate(("pit", "log_cdf", "log_sf", "mean_resid")):
            assert np.array_equal(t[:, 5 + j], f12(d[key])), key
