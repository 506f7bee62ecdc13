"""bin/chainsummary_hip --scan on the GPU: the 23-sample chain of summary_support.stored_chain on the golden local-model
inputs.  --scan 7,20 writes <output file>.scan and <output file>.scan.regions, whose 17-digit numbers
parse back to the bits of Summary(..., scan=(7, 20)).scan_result(k) and .scan_regions(k, which, line), at the default line and
with --scan-below; the output file and <output file>.windows are, byte for byte, what the same binary writes without the
flag."""
import os
import subprocess

import numpy as np
import pytest

from summary_support import header_values, stored_chain
from support import bits
from tamcmc_amd import capi

pytestmark = pytest.mark.gpu


def test_command_line(accel_mod, tmp_path):
    s, root, v, rows, common, sel = stored_chain(tmp_path)
    with accel_mod.Accel(s.model_case, s.plength, s.x, s.y, sigma_y=s.sigma_y, likelihood_case=s.likelihood_case,
                         likelihood_p=s.likelihood_p) as acc:
        with capi.Summary(acc, scan=(7, 20)) as sm:
            _, st = sm.push(rows)
            d = [sm.scan_result(k) for k in range(2)]
            line = float(np.median(d[1]["log_sf"]))
            assert line < 0
            regs = {below: [(W, which, r) for k, W in enumerate((7, 20)) for which in (0, 1) for r in sm.scan_regions(k, which, below)]
                    for below in (None, line)}
    assert np.all(st == 0) and d[0]["n_used"] == 23 and d[1]["n_positions"] == s.Nx - 19 and len(regs[line]) >= 1
    plain, table = str(tmp_path / "plain.txt"), str(tmp_path / "scan.txt")
    for path, flag in ((plain, []), (table, ["--scan", "7,20"])):
        r = subprocess.run(common + [path] + sel + ["--window", "7,3", "--predictive"] + flag, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
    assert open(table, "rb").read() == open(plain, "rb").read(), "the output file changed with --scan"
    assert open(table + ".windows", "rb").read() == open(plain + ".windows", "rb").read(), ".windows changed with --scan"
    assert not os.path.exists(plain + ".scan") and not os.path.exists(plain + ".scan.regions")
    lines = open(table + ".scan").read().split("\n")
    head = [ln for ln in lines if ln.startswith("#")]
    assert lines[:len(head)] == head and lines[-1] == "" and len(lines) == len(head) + s.Nx + 1
    assert head[0].startswith("# chainsummary_hip (") and head[1] == "# widths= 7,20" and head[2] == "# n_used= 23  n_rejected= 0"
    assert len(head) == 6 and head[-1].startswith("# j x pit_7 log_cdf_7 log_sf_7 mean_resid_7 pit_20 ")
    for k in range(2):
        val = header_values([head[3 + k]])
        for key in ("W", "n_positions", "pos_min_log_sf", "pos_min_log_cdf"):
            assert int(val[key]) == d[k][key], (k, key)
        for key in ("min_log_sf", "min_log_cdf"):
            assert np.array_equal(bits(float(val[key])), bits(float(d[k][key]))), (k, key)
    t = np.loadtxt(table + ".scan")
    assert t.shape == (s.Nx, 10) and np.array_equal(t[:, 0], np.arange(s.Nx)) and np.array_equal(bits(t[:, 1]), bits(np.asarray(s.x, dtype=np.float64)))
    for k in range(2):
        n_pos = d[k]["n_positions"]
        for j, key in enumerate(capi.Summary.SCAN_ARRAYS):
            col = t[:, 2 + 4 * k + j]
            assert np.array_equal(bits(col[:n_pos]), bits(d[k][key])), (k, key)
            assert np.all(np.isnan(col[n_pos:])) and len(col[n_pos:]) == (6, 19)[k]

    def check_regions(path, want):
        lines = open(path).read().split("\n")
        head = [ln for ln in lines if ln.startswith("#")]
        assert lines[:len(head)] == head and lines[-1] == "" and len(lines) == len(head) + len(want) + 1
        assert head[-1] == "# W which pos_first pos_last bin_first bin_last x_first x_last pos_min min_log mean_resid_at_min"
        for ln, (W, which, r) in zip(lines[len(head):-1], want):
            tok = ln.split()
            assert [int(v) for v in tok[:6]] == [W, which, r["pos_first"], r["pos_last"], r["bin_first"], r["bin_last"]] and int(tok[8]) == r["pos_min"]
            got = np.array([float(v) for v in (tok[6], tok[7], tok[9], tok[10])])
            assert np.array_equal(bits(got), bits(np.array([s.x[r["bin_first"]], s.x[r["bin_last"]], r["min_log"], r["mean_resid_at_min"]])))

    check_regions(table + ".scan.regions", regs[None])
    below = str(tmp_path / "below.txt")
    r = subprocess.run(common + [below] + sel + ["--scan", "7,20", "--scan-below", "%.17g" % line], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(below + ".scan", "rb").read() == open(table + ".scan", "rb").read()
    check_regions(below + ".scan.regions", regs[line])
