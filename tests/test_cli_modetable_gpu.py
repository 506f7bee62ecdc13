"""chainsummary_hip --modes [q1,q2,...] on the GPU: the stored chain of summary_support.stored_chain on the golden local-model
inputs.  <output file>.modes parses -- the totals in its header, one row per column of the mode table -- and its numbers,
printed with 17 significant digits, parse back to the bits ModeTable returns for the same samples, with --thin and
--first (and --last) applied; the main output file is, byte for byte, what the same binary writes without the flag."""
import os
import subprocess

import numpy as np
import pytest

from summary_support import header_values, stored_chain
from support import bits
from tamcmc_amd import capi

pytestmark = pytest.mark.gpu

QS = [0.16, 0.5, 0.84]


def test_command_line(accel_mod, tmp_path):
    s, root, v, rows, common, sel = stored_chain(tmp_path)
    want = {}
    with accel_mod.Accel(s.model_case, s.plength, s.x, s.y, sigma_y=s.sigma_y, likelihood_case=s.likelihood_case,
                         likelihood_p=s.likelihood_p) as acc:
        with capi.Summary(acc) as sm:
            _, st = sm.push(rows)
        assert np.all(st == 0)
        for tag, sub, q in (("all", rows, QS), ("last", rows[:19], QS), ("default", rows, QS), ("two", rows, [0.025, 0.975])):
            with capi.ModeTable(acc, len(sub)) as mt:
                cols = mt.columns()
                mt.push(sub)
                want[tag] = dict(mt.result(), q=mt.quantiles(q)["values"], cols=cols)
    plain = str(tmp_path / "plain.txt")
    r = subprocess.run(common + [plain] + sel, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert not os.path.exists(plain + ".modes")
    plain_last = str(tmp_path / "plain_last.txt")
    r = subprocess.run(common + [plain_last] + sel + ["--last", "40"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for tag, flags, ref_file, qtext in (("all", ["--modes", "0.16,0.5,0.84"], plain, "0.16,0.5,0.84"),
                                        ("last", ["--last", "40", "--modes", "0.16,0.5,0.84"], plain_last, "0.16,0.5,0.84"),
                                        ("default", ["--modes"], plain, "0.16,0.5,0.84"),
                                        ("two", ["--modes", "0.025,0.975"], plain, "0.025,0.975")):
        table = str(tmp_path / f"modes_{tag}.txt")
        r = subprocess.run(common + [table] + sel + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert open(table, "rb").read().replace(table.encode(), b"@") == open(ref_file, "rb").read().replace(ref_file.encode(), b"@"), \
            "the output file changed with --modes"
        d = want[tag]
        nq = d["q"].shape[0]
        lines = open(table + ".modes").read().split("\n")
        head = header_values(line for line in lines if line.startswith("#") and "=" in line)
        assert lines[0].startswith("# chainsummary_hip (") and head["quantiles"] == qtext
        assert lines[3].split()[:12] == "# col kind mult order l m param_index mean sd min max".split() and len(lines[3].split()) == 12 + nq
        for k in ("n_used", "n_rejected", "n_cols", "n_mult"):
            assert int(head[k]) == d[k], k
        body = [line.split() for line in lines[4:] if line]
        assert len(body) == d["n_cols"]
        for k, tok in enumerate(body):
            c = d["cols"][k]
            assert int(tok[0]) == k and tok[1] == capi.MODETABLE_KINDS[c["kind"]]
            assert [int(t) for t in tok[2:7]] == [c["mult"], c["order"], c["l"], c["m"], c["param_index"]]
            got = np.array([float(t) for t in tok[7:]])
            ref = np.concatenate([[d["mean"][k], d["sd"][k], d["min"][k], d["max"][k]], d["q"][:, k]])
            assert np.array_equal(bits(got), bits(ref)), (tag, k, got, ref)
