"""bin/chainsummary_hip --predictive on the GPU: the 23-sample chain of summary_support.stored_chain on the golden
local-model inputs, with and without --loo.  Two more header lines and four last columns, the numbers
Summary.predictive_result() gives to the 12 printed digits; everything else is, byte for byte, what the same binary writes
without the flag."""
import subprocess

import numpy as np
import pytest

from summary_support import f12, header_values, stored_chain
from tamcmc_amd import capi

pytestmark = pytest.mark.gpu

COLS = " pit log_cdf log_sf mean_resid"


def test_command_line(accel_mod, tmp_path):
    s, root, v, rows, common, sel = stored_chain(tmp_path)
    with accel_mod.Accel(s.model_case, s.plength, s.x, s.y, sigma_y=s.sigma_y, likelihood_case=s.likelihood_case,
                         likelihood_p=s.likelihood_p) as acc:
        with capi.Summary(acc, predictive=True) as sm:
            _, st = sm.push(rows)
            d = sm.predictive_result()
    assert np.all(st == 0) and d["n_used"] == 23
    for extra, ncol in (([], 8), (["--loo"], 10), (["--quantiles", "0.16,0.5,0.84", "--loo"], 13)):
        plain, table = str(tmp_path / f"plain{ncol}.txt"), str(tmp_path / f"pred{ncol}.txt")
        for path, flag in ((plain, []), (table, ["--predictive"])):
            r = subprocess.run(common + [path] + sel + extra + flag, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout + r.stderr
        t = np.loadtxt(table)
        assert t.shape == (s.Nx, ncol + 4)
        for j, key in enumerate(("pit", "log_cdf", "log_sf", "mean_resid")):
            assert np.array_equal(t[:, ncol + j], f12(d[key])), key
        lines0, lines = open(plain).read().split("\n"), open(table).read().split("\n")
        added = [k for k, line in enumerate(lines) if line.startswith("# ks_D=") or line.startswith("# pit_hist=")]
        assert len(added) == 2 and added[1] == added[0] + 1 and lines[added[1] + 1].startswith("# x y ")
        assert lines[added[0] - 1].startswith("# elpd_loo=" if extra else "# lppd_total=")
        head = header_values([lines[added[0]]])
        for key in ("ks_D", "min_log_sf", "min_log_cdf"):
            assert head[key] == "%.12g" % d[key], key
        assert int(head["bin_min_log_sf"]) == d["bin_min_log_sf"] and int(head["bin_min_log_cdf"]) == d["bin_min_log_cdf"]
        hist = [int(c) for c in lines[added[1]].split("=")[1].split()]
        assert hist == list(d["pit_hist"]) and sum(hist) == s.Nx
        # minus the two added lines and the four columns: the bytes of the run without the flag
        stripped = []
        for k, line in enumerate(lines):
            if k in added:
                continue
            if line.startswith("# x y "):
                assert line.endswith(COLS)
                line = line[:-len(COLS)]
            elif line and not line.startswith("#"):
                line = line.rsplit(" ", 4)[0]
            stripped.append(line)
        assert stripped == lines0, "the output without --predictive changed"
