"""chainsummary_hip --modes --modes-ess [L] --modes-corr on the GPU: the stored chain of summary_support.stored_chain on the
golden local-model inputs.  <output file>.modes.ess and <output file>.modes.corr parse -- the totals in their headers, one
row per column of the mode table, the matrix of the headline columns -- and their numbers, printed with 17 significant
digits, parse back to the bits ModeTable.ess() and ModeTable.corr(headline columns) return for the same samples, with --thin
and --first (and --last) applied; the main output file and .modes are, byte for byte, what the same binary writes without
the new flags, and neither new file exists without its flag."""
import os
import subprocess

import numpy as np
import pytest

import modediag_reference as DR
from summary_support import header_values, stored_chain
from support import bits
from tamcmc_amd import capi

pytestmark = pytest.mark.gpu


def same_file(a, b):
    return open(a, "rb").read().replace(a.encode(), b"@") == open(b, "rb").read().replace(b.encode(), b"@")


def test_command_line(accel_mod, tmp_path):
    s, root, v, rows, common, sel = stored_chain(tmp_path)
    want = {}
    with accel_mod.Accel(s.model_case, s.plength, s.x, s.y, sigma_y=s.sigma_y, likelihood_case=s.likelihood_case,
                         likelihood_p=s.likelihood_p) as acc:
        with capi.Summary(acc) as sm:
            _, st = sm.push(rows)
        assert np.all(st == 0)
        for tag, sub, lag in (("all", rows, 0), ("last", rows[:19], 0), ("lag15", rows, 15)):
            with capi.ModeTable(acc, len(sub)) as mt:
                cols = mt.columns()
                mt.push(sub)
                head = DR.headline(cols)
                want[tag] = dict(mt.ess(lag), totals=mt.result(), cols=cols, head=head, corr=mt.corr(head))
    assert len(want["all"]["head"]) == 4 + 5 * want["all"]["totals"]["n_mult"]
    plain = str(tmp_path / "plain.txt")
    r = subprocess.run(common + [plain] + sel + ["--modes"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(plain + ".modes") and not os.path.exists(plain + ".modes.ess") and not os.path.exists(plain + ".modes.corr")
    plain_last = str(tmp_path / "plain_last.txt")
    r = subprocess.run(common + [plain_last] + sel + ["--last", "40", "--modes"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for tag, flags, ref_file, has_ess, has_corr, lag in (
            ("all", ["--modes", "--modes-ess", "--modes-corr"], plain, True, True, 21),
            ("last", ["--last", "40", "--modes-corr", "--modes", "--modes-ess", "0"], plain_last, True, True, 17),
            ("lag15", ["--modes", "--modes-ess", "15"], plain, True, False, 15),
            ("all", ["--modes-corr", "--modes"], plain, False, True, None)):
        out = str(tmp_path / f"diag_{tag}_{int(has_ess)}{int(has_corr)}.txt")
        r = subprocess.run(common + [out] + sel + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert same_file(out, ref_file), "the output file changed with the new flags"
        assert same_file(out + ".modes", ref_file + ".modes"), ".modes changed with the new flags"
        assert os.path.exists(out + ".modes.ess") == has_ess and os.path.exists(out + ".modes.corr") == has_corr, flags
        d = want[tag]
        if has_ess:
            lines = open(out + ".modes.ess").read().split("\n")
            head = header_values(line for line in lines if line.startswith("#") and "=" in line)
            assert lines[0].startswith("# chainsummary_hip (") and lines[0] == open(out + ".modes").readline().rstrip("\n")
            assert lines[3] == "# col kind mult order l m param_index ess tau mcse rhat cut"
            for k in ("n_used", "n_rejected", "n_cols", "n_mult"):
                assert int(head[k]) == d["totals"][k], k
            assert int(head["lag"]) == d["lag"] == lag
            for k in ("col_min_ess", "col_max_rhat", "n_truncated", "n_constant", "n_rhat_high"):
                assert int(head[k]) == d[k], k
            for k in ("min_ess", "max_rhat"):
                assert bits(float(head[k])) == bits(d[k]), k
            body = [line.split() for line in lines[4:] if line]
            assert len(body) == d["totals"]["n_cols"]
            for k, tok in enumerate(body):
                c = d["cols"][k]
                assert int(tok[0]) == k and tok[1] == capi.MODETABLE_KINDS[c["kind"]]
                assert [int(t) for t in tok[2:7]] == [c["mult"], c["order"], c["l"], c["m"], c["param_index"]]
                got = np.array([float(t) for t in tok[7:11]])
                ref = np.array([d["ess"][k], d["tau"][k], d["mcse"][k], d["rhat"][k]])
                assert np.array_equal(bits(got), bits(ref)) or (np.array_equal(np.isnan(got), np.isnan(ref)) and
                                                                np.array_equal(bits(got[~np.isnan(got)]), bits(ref[~np.isnan(ref)]))), (tag, k, got, ref)
                assert int(tok[11]) == d["cut"][k] and len(tok) == 12
        if has_corr:
            lines = open(out + ".modes.corr").read().split("\n")
            head = header_values(line for line in lines if line.startswith("#") and "= " in line and not line.startswith("# cols"))
            assert lines[0].startswith("# chainsummary_hip (") and int(head["n_used"]) == d["totals"]["n_used"] and int(head["n_cols"]) == d["totals"]["n_cols"]
            assert lines[2].startswith("# cols = ") and [int(t) for t in lines[2][len("# cols = "):].split()] == list(d["head"])
            got = np.array([[float(t) for t in line.split()] for line in lines[3:] if line])
            assert got.shape == d["corr"].shape
            nan = np.isnan(d["corr"])
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(d["corr"][~nan])), tag
            assert nan.any() and np.all(np.diag(got)[~np.diag(nan)] == 1.0)      # (splitting of the l = 0 modes is constant)
