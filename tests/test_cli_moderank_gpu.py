"""chainsummary_hip --modes --modes-rank [L] on the GPU: the stored chain of summary_support.stored_chain on the golden
local-model inputs.  <output file>.modes.rank parses -- the totals in its header, one row per column of the mode table in the
order of .modes.ess -- and its numbers, printed with 17 significant digits, parse back to the bits ModeTable.rank_diag()
returns for the same samples, with --thin and --first (and --last) applied; the main output file, .modes and .modes.ess are,
byte for byte, what the same binary writes without the new flag, .modes.rank does not exist without it, and --modes-rank
without --modes prints the usage text."""
import os
import subprocess

import numpy as np
import pytest

import moderank_reference as RR
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
        for tag, sub, lag in (("all", rows, 0), ("last", rows[:19], 0), ("lag15", rows, 15)):
            with capi.ModeTable(acc, len(sub)) as mt:
                cols = mt.columns()
                mt.push(sub)
                want[tag] = dict(mt.rank_diag(lag), totals=mt.result(), columns=cols)
    plain = str(tmp_path / "plain.txt")
    r = subprocess.run(common + [plain] + sel + ["--modes", "--modes-ess"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(plain + ".modes") and os.path.exists(plain + ".modes.ess") and not os.path.exists(plain + ".modes.rank")
    plain_last = str(tmp_path / "plain_last.txt")
    r = subprocess.run(common + [plain_last] + sel + ["--last", "40", "--modes", "--modes-ess"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run(common + [str(tmp_path / "none.txt")] + sel + ["--modes-rank"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr and "--modes-rank needs --modes" in r.stderr
    assert not os.path.exists(str(tmp_path / "none.txt"))
    for tag, flags, ref_file, lag in (("all", ["--modes", "--modes-ess", "--modes-rank"], plain, 21),
                                      ("last", ["--last", "40", "--modes-rank", "0", "--modes", "--modes-ess"], plain_last, 17),
                                      ("lag15", ["--modes-rank", "15", "--modes", "--modes-ess"], plain, 15)):
        out = str(tmp_path / f"rank_{tag}.txt")
        r = subprocess.run(common + [out] + sel + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert same_file(out, ref_file), "the output file changed with the new flag"
        assert same_file(out + ".modes", ref_file + ".modes") and same_file(out + ".modes.ess", ref_file + ".modes.ess"), "a .modes file changed"
        d = want[tag]
        lines = open(out + ".modes.rank").read().split("\n")
        head = header_values(line for line in lines if line.startswith("#") and "=" in line)
        assert lines[0].startswith("# chainsummary_hip (") and lines[0] == open(out + ".modes").readline().rstrip("\n")
        assert lines[3] == "# col kind mult order l m param_index " + " ".join(RR.OUT) + " cut_z cut_zfold cut_i05 cut_i95"
        for k in ("n_used", "n_rejected", "n_cols", "n_mult"):
            assert int(head[k]) == d["totals"][k], k
        assert int(head["lag"]) == d["lag"] == lag
        for k in RR.TOTALS[3:]:
            if k.startswith(("min_", "max_")):
                assert bits(float(head[k])) == bits(d[k]), k
            else:
                assert int(head[k]) == d[k], k
        body = [line.split() for line in lines[4:] if line]
        ess_body = [line.split() for line in open(out + ".modes.ess").read().split("\n")[4:] if line]
        assert len(body) == d["totals"]["n_cols"] == len(ess_body)
        for k, tok in enumerate(body):
            c = d["columns"][k]
            assert tok[:7] == ess_body[k][:7] and int(tok[0]) == k and tok[1] == capi.MODETABLE_KINDS[c["kind"]]
            got = np.array([float(t) for t in tok[7:15]])
            ref = np.array([d[name][k] for name in RR.OUT])
            assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(bits(got[~np.isnan(got)]), bits(ref[~np.isnan(ref)])), (tag, k, got, ref)
            assert [int(t) for t in tok[15:]] == list(d["cut"][:, k]) and len(tok) == 19
