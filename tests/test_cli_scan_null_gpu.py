"""bin/chainsummary_hip --scan-null on the GPU: the 23-sample chain of tests/test_cli_scan_gpu.py on the golden local-model
inputs.  Without the flag nothing is said about a null: the output file, .scan and .scan.regions are what --scan alone writes
(tests/test_cli_scan_gpu.py pins their content).  With --scan-null R,seed the output file and .scan keep every byte, and
.scan.regions carries the line `# null= R seed alpha= 0.01 joint_line= ...` and the two trailing columns p_width p_joint,
whose 17-digit numbers parse back to the bits of ScanNull(...).line(k, which, 0.01, True) and .pvalue(k, which, min_log); the
regions are those of Summary.scan_regions at the joint line, or at T with --scan-below T."""
import subprocess

import numpy as np
import pytest

from summary_support import stored_chain
from support import bits
from tamcmc_amd import capi

pytestmark = pytest.mark.gpu

WIDTHS, R_NULL, SEED = (7, 20), 300, 9


def test_command_line(accel_mod, tmp_path):
    s, root, v, rows, common, sel = stored_chain(tmp_path)
    with accel_mod.ScanNull(s.likelihood_case, s.likelihood_p, s.Nx, WIDTHS, SEED) as null:
        null.run(R_NULL)
        joint = [null.line(k, which, 0.01, True) for k in range(2) for which in (0, 1)]
        with accel_mod.Accel(s.model_case, s.plength, s.x, s.y, sigma_y=s.sigma_y, likelihood_case=s.likelihood_case,
                             likelihood_p=s.likelihood_p) as acc:
            with capi.Summary(acc, scan=WIDTHS) as sm:
                sm.push(rows)
                T = float(np.median(sm.scan_result(1)["log_sf"]))
                assert T < 0
                want = {}
                for tag, line_of in (("joint", lambda k, which: joint[2 * k + which]), ("below", lambda k, which: T)):
                    want[tag] = [(W, which, r, null.pvalue(k, which, r["min_log"]))
                                 for k, W in enumerate(WIDTHS) for which in (0, 1) for r in sm.scan_regions(k, which, line_of(k, which))]
    assert len(want["below"]) >= 1
    plain, table, below = str(tmp_path / "plain.txt"), str(tmp_path / "null.txt"), str(tmp_path / "below.txt")
    flag = ["--scan-null", f"{R_NULL},{SEED}"]
    for path, extra in ((plain, []), (table, flag), (below, flag + ["--scan-below", "%.17g" % T])):
        r = subprocess.run(common + [path] + sel + ["--scan", "7,20"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
    for path in (table, below):
        assert open(path, "rb").read() == open(plain, "rb").read(), "the output file changed with --scan-null"
        assert open(path + ".scan", "rb").read() == open(plain + ".scan", "rb").read(), ".scan changed with --scan-null"
    plain_head = [ln for ln in open(plain + ".scan.regions").read().split("\n") if ln.startswith("#")]
    assert len(plain_head) == 3 and not any("null=" in ln or "p_width" in ln for ln in plain_head)
    assert plain_head[-1] == "# W which pos_first pos_last bin_first bin_last x_first x_last pos_min min_log mean_resid_at_min"

    def check(path, regs, lines_in_use):
        lines = open(path).read().split("\n")
        head = [ln for ln in lines if ln.startswith("#")]
        assert lines[:len(head)] == head and lines[-1] == "" and len(lines) == len(head) + len(regs) + 1
        assert len(head) == 4 and head[0] == plain_head[0]
        tok = head[1].split()
        assert tok[:4] == ["#", "widths=", "7,20", "log_below="] and np.array_equal(bits([float(v) for v in tok[4:]]), bits(lines_in_use))
        tok = head[2].split()
        assert tok[:6] == ["#", "null=", str(R_NULL), str(SEED), "alpha=", "0.01"] and tok[6] == "joint_line=" and len(tok) == 11
        assert np.array_equal(bits([float(v) for v in tok[7:]]), bits(joint))
        assert head[3] == plain_head[-1] + " p_width p_joint"
        for ln, (W, which, r, pv) in zip(lines[len(head):-1], regs):
            tok = ln.split()
            assert len(tok) == 13
            assert [int(v) for v in tok[:6]] == [W, which, r["pos_first"], r["pos_last"], r["bin_first"], r["bin_last"]] and int(tok[8]) == r["pos_min"]
            got = np.array([float(v) for v in (tok[6], tok[7], tok[9], tok[10], tok[11], tok[12])])
            assert np.array_equal(bits(got), bits(np.array([s.x[r["bin_first"]], s.x[r["bin_last"]], r["min_log"], r["mean_resid_at_min"], pv[0], pv[1]])))

    check(table + ".scan.regions", want["joint"], joint)
    check(below + ".scan.regions", want["below"], [T, T])
    # the rows of the --scan-below run are those of the same run without the null, plus the two columns
    r = subprocess.run(common + [plain] + sel + ["--scan", "7,20", "--scan-below", "%.17g" % T], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    a = [ln for ln in open(plain + ".scan.regions").read().split("\n") if ln and not ln.startswith("#")]
    b = [ln for ln in open(below + ".scan.regions").read().split("\n") if ln and not ln.startswith("#")]
    assert len(a) == len(b) and all(y.startswith(x + " ") and len(y[len(x):].split()) == 2 for x, y in zip(a, b))
