"""chainsummary_hip --loo-pit on the GPU: the 23-sample chain of summary_support.stored_chain on the golden local-model
inputs.  <output file>.loopit parses -- the totals in its header, one row per bin -- and holds the numbers
Summary.loo(rows, pit=True) gives, to the 12 printed digits; the option implies --loo, so the main output file is, byte for
byte, what the same binary writes with --loo alone, and without the option no .loopit file appears."""
import os
import subprocess

import numpy as np
import pytest

from summary_support import f12, header_values, stored_chain
from tamcmc_amd import capi

pytestmark = pytest.mark.gpu

COLUMNS = ("x", "loo_pit", "loo_log_cdf", "loo_log_sf", "is_ess", "pareto_k")


def test_command_line(accel_mod, tmp_path):
    s, root, v, rows, common, sel = stored_chain(tmp_path)
    with accel_mod.Accel(s.model_case, s.plength, s.x, s.y, sigma_y=s.sigma_y, likelihood_case=s.likelihood_case,
                         likelihood_p=s.likelihood_p) as acc:
        with capi.Summary(acc) as sm:
            _, st = sm.push(rows)
            d = sm.loo(rows, pit=True)
    assert np.all(st == 0) and d["n_used"] == 23 and d["n_rejected"] == 0
    plain = str(tmp_path / "plain.txt")
    r = subprocess.run(common + [plain] + sel + ["--loo"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert not os.path.exists(plain + ".loopit")
    for flags in (["--loo-pit"], ["--loo", "--loo-pit"]):
        table = str(tmp_path / ("pit%d.txt" % len(flags)))
        r = subprocess.run(common + [table] + sel + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert open(table, "rb").read().replace(table.encode(), b"@") == open(plain, "rb").read().replace(plain.encode(), b"@"), \
            "the output file is not that of --loo"
        lines = open(table + ".loopit").read().split("\n")
        head = header_values(line for line in lines if line.startswith("#") and "=" in line)
        assert lines[0].startswith("# chainsummary_hip (") and lines[5] == "# " + " ".join(COLUMNS)
        for k, name in (("n_used", "n_used"), ("n_rejected", "n_rejected"), ("bin_min_log_sf", "bin_min_loo_log_sf"),
                        ("bin_min_log_cdf", "bin_min_loo_log_cdf"), ("bin_min_is_ess", "bin_min_is_ess")):
            assert int(head[k]) == d[name], k
        for k, name in (("ks_D", "loo_ks_D"), ("min_log_sf", "min_loo_log_sf"), ("min_log_cdf", "min_loo_log_cdf"), ("min_is_ess", "min_is_ess")):
            assert head[k] == "%.12g" % d[name], k
        assert [int(t) for t in lines[4].split("=")[1].split()] == list(d["loo_pit_hist"]) and sum(d["loo_pit_hist"]) == s.Nx
        t = np.loadtxt(table + ".loopit")
        assert t.shape == (s.Nx, len(COLUMNS))
        assert np.array_equal(t[:, 0], f12(s.x))
        for j, k in enumerate(COLUMNS[1:], start=1):
            assert np.array_equal(t[:, j], f12(d[k]), equal_nan=True), k
