"""chainsummary_hip --quantiles 0.025,0.5,0.975 --band-ess 7 on the GPU: the 23-sample chain of summary_support.stored_chain on
the golden local-model inputs.  <output file>.bandess is written, parses -- the totals per quantile in its header, one row per
bin -- and holds the numbers Summary.band_ess gives on the same 23 rows, to the 12 printed digits; its header totals are
consistent with its columns; and the main output file is, byte for byte, what the same binary writes for --quantiles alone."""
import os
import subprocess

import numpy as np
import pytest

from summary_support import f12, header_values, stored_chain
from tamcmc_amd import capi

pytestmark = pytest.mark.gpu

Q = (0.025, 0.5, 0.975)
PER_Q = ("value", "count_le", "p_hat", "ess", "tau", "mcse_p", "cut")


def test_command_line(accel_mod, tmp_path):
    s, root, v, rows, common, sel = stored_chain(tmp_path)
    with accel_mod.Accel(s.model_case, s.plength, s.x, s.y, sigma_y=s.sigma_y, likelihood_case=s.likelihood_case,
                         likelihood_p=s.likelihood_p) as acc:
        with capi.Summary(acc) as sm:
            _, st = sm.push(rows)
            want = sm.band_ess(rows, Q, 7)
    assert np.all(st == 0) and want["n_used"] == 23 and want["lag"] == 7 and want["bits_left"] == 0
    quant = ["--quantiles", ",".join("%g" % q for q in Q)]
    plain = str(tmp_path / "plain.txt")
    r = subprocess.run(common + [plain] + sel + quant, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert not os.path.exists(plain + ".bandess")
    table = str(tmp_path / "band.txt")
    r = subprocess.run(common + [table] + sel + quant + ["--band-ess", "7"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(table, "rb").read().replace(table.encode(), b"@") == open(plain, "rb").read().replace(plain.encode(), b"@"), \
        "the output file changed with --band-ess"
    assert os.path.exists(table + ".bandess")
    assert not os.path.exists(table + ".ess"), "--band-ess wrote another mode's file"
    lines = open(table + ".bandess").read().split("\n")
    assert lines[0].startswith("# chainsummary_hip (") and lines[1] == "# quantiles= 0.025,0.5,0.975"
    head = header_values(lines[2:3])
    assert int(head["n_used"]) == 23 and int(head["n_rejected"]) == 0 and int(head["lag"]) == 7
    names = lines[6][2:].split()
    assert lines[6].startswith("# x ") and names == ["x"] + ["q%g" % q if k == "value" else "%s_%g" % (k, q) for q in Q for k in PER_Q]
    t = np.loadtxt(table + ".bandess")
    assert t.shape == (s.Nx, 1 + len(Q) * len(PER_Q))
    assert np.array_equal(t[:, 0], f12(s.x))
    for j, q in enumerate(Q):
        col = {k: t[:, 1 + j * len(PER_Q) + i] for i, k in enumerate(PER_Q)}
        assert np.array_equal(col["value"], f12(want["lo"][j])), q
        for k in PER_Q[1:]:
            assert np.array_equal(col[k], f12(want[k][j]), equal_nan=True), (q, k)
        # the header's totals for this quantile: the library's, and consistent with the file's own columns
        h = header_values(lines[3 + j:4 + j])
        assert h["q"] == "%.6g" % q
        assert h["min_ess"] == "%.12g" % want["min_ess"][j] and int(h["bin_min_ess"]) == want["bin_min_ess"][j]
        assert int(h["n_truncated"]) == want["n_truncated"][j] == int((col["cut"] == 8).sum())
        assert int(h["n_constant"]) == want["n_constant"][j] == int(((col["count_le"] == 0) | (col["count_le"] == 23)).sum())
        if want["bin_min_ess"][j] >= 0:
            assert float(h["min_ess"]) == np.nanmin(col["ess"]) and col["ess"][int(h["bin_min_ess"])] == np.nanmin(col["ess"])
        assert np.all(col["count_le"] >= np.ceil(q * 23)) and np.array_equal(col["p_hat"], f12(col["count_le"] / 23.0))
