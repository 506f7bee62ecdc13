"""chainsummary_hip --ess [L] on the GPU: the 23-sample chain of summary_support.stored_chain on the golden local-model
inputs.  <output file>.ess parses -- the totals in its header, one row per bin -- and holds the numbers
Summary.ess gives, to the 12 printed digits, with the default lag limit and with --ess 31 (both resolve to the chain's own
limit, 21); the main output file is, byte for byte, what the same binary writes without the flag."""
import os
import subprocess

import numpy as np
import pytest

from summary_support import f12, header_values, stored_chain
from tamcmc_amd import capi

pytestmark = pytest.mark.gpu

COLUMNS = ("x", "ess_M", "tau_M", "mcse_M", "rhat_M", "cut_M", "ess_l", "r_eff", "cut_l")


def test_command_line(accel_mod, tmp_path):
    s, root, v, rows, common, sel = stored_chain(tmp_path)
    with accel_mod.Accel(s.model_case, s.plength, s.x, s.y, sigma_y=s.sigma_y, likelihood_case=s.likelihood_case,
                         likelihood_p=s.likelihood_p) as acc:
        with capi.Summary(acc) as sm:
            _, st = sm.push(rows)
            want = {0: sm.ess(rows), 31: sm.ess(rows, 31), 5: sm.ess(rows, 5)}
    assert np.all(st == 0) and want[0]["n_used"] == 23 and want[0]["lag"] == 21 and want[31]["lag"] == 21 and want[5]["lag"] == 5
    plain = str(tmp_path / "plain.txt")
    r = subprocess.run(common + [plain] + sel + ["--loo"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert not os.path.exists(plain + ".ess")
    for lag, flag in ((0, ["--ess"]), (31, ["--ess", "31"]), (5, ["--ess", "5"])):
        table = str(tmp_path / f"ess{lag}.txt")
        r = subprocess.run(common + [table] + sel + flag + ["--loo"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert open(table, "rb").read().replace(table.encode(), b"@") == open(plain, "rb").read().replace(plain.encode(), b"@"), \
            "the output file changed with --ess"
        d = want[lag]
        lines = open(table + ".ess").read().split("\n")
        head = header_values(line for line in lines if line.startswith("#") and "=" in line)
        assert lines[0].startswith("# chainsummary_hip (") and lines[5] == "# " + " ".join(COLUMNS)
        for k in ("n_used", "n_rejected", "lag", "bin_min_ess_M", "bin_min_ess_l", "bin_max_rhat", "n_rhat_high", "n_truncated_M", "n_truncated_l"):
            assert int(head[k]) == d[k], k
        for k in ("min_ess_M", "min_ess_l", "max_rhat"):
            assert head[k] == "%.12g" % d[k], k
        t = np.loadtxt(table + ".ess")
        assert t.shape == (s.Nx, len(COLUMNS))
        assert np.array_equal(t[:, 0], f12(s.x))
        for j, k in enumerate(COLUMNS[1:], start=1):
            assert np.array_equal(t[:, j], f12(d[k]), equal_nan=True), (lag, k)
