"""chainsummary_hip --modes --modes-hist [N] --modes-hpd m1[,m2...] --modes-pairs c1:c2[,...] [N] on the GPU: the stored chain
of summary_support.stored_chain on the golden local-model inputs.  The three files parse; their integers are those of
ModeTable.hist / hpd / hist2d for the same samples and their doubles, printed with 17 significant digits, parse back to the
same bits; the main output file and .modes are, byte for byte, what the same binary writes without the new flags, and none
of the three files exists without its flag."""
import os
import subprocess

import numpy as np
import pytest

from summary_support import header_values, stored_chain
from support import bits
from tamcmc_amd import capi

pytestmark = pytest.mark.gpu

PAIRS = [[5, 6], [4, 4], [0, 7]]
MASS = [0.68, 0.95]


def same_file(a, b):
    return open(a, "rb").read().replace(a.encode(), b"@") == open(b, "rb").read().replace(b.encode(), b"@")


def test_command_line(accel_mod, tmp_path):
    s, root, v, rows, common, sel = stored_chain(tmp_path)
    with accel_mod.Accel(s.model_case, s.plength, s.x, s.y, sigma_y=s.sigma_y, likelihood_case=s.likelihood_case,
                         likelihood_p=s.likelihood_p) as acc, capi.ModeTable(acc, len(rows)) as mt:
        cols = mt.columns()
        mt.push(rows)
        totals = mt.result()
        want = dict(h50=mt.hist(50), h7=mt.hist(7), p=mt.hpd(MASS), med=mt.quantiles([0.5])["values"][0],
                    j32=mt.hist2d(PAIRS, 32, mass=(0.68, 0.95)), j5=mt.hist2d(PAIRS, 5, mass=(0.68, 0.95)))
    nc = totals["n_cols"]
    plain = str(tmp_path / "plain.txt")
    r = subprocess.run(common + [plain] + sel + ["--modes"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for ext in (".hist", ".hpd", ".pairs"):
        assert os.path.exists(plain + ".modes") and not os.path.exists(plain + ".modes" + ext)
    r = subprocess.run(common + [str(tmp_path / "none.txt")] + sel + ["--modes-hist"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr and "need --modes" in r.stderr and not os.path.exists(str(tmp_path / "none.txt"))
    pair_text = ",".join("%d:%d" % tuple(p) for p in PAIRS)
    for tag, flags, hkey, jkey, nb, nb2 in (("default", ["--modes", "--modes-hist", "--modes-hpd", "0.68,0.95", "--modes-pairs", pair_text], "h50", "j32", 50, 32),
                                            ("given", ["--modes-pairs", pair_text, "5", "--modes-hpd", "0.68,0.95", "--modes-hist", "7", "--modes"], "h7", "j5", 7, 5)):
        out = str(tmp_path / f"pdf_{tag}.txt")
        r = subprocess.run(common + [out] + sel + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert same_file(out, plain) and same_file(out + ".modes", plain + ".modes"), "an existing file changed with the new flags"
        first = open(out + ".modes").readline().rstrip("\n")
        # ---- .modes.hist ----
        lines = open(out + ".modes.hist").read().split("\n")
        head = header_values(lines[1:3])
        assert lines[0] == first and int(head["n_used"]) == totals["n_used"] and int(head["n_cols"]) == nc and int(head["n_bins"]) == nb
        h = want[hkey]
        body = lines[3:]
        per = 3 + nb + 1
        assert len([x for x in body if x]) == nc * per
        for k in range(nc):
            blk = body[k * per:(k + 1) * per]
            tok = blk[0].split()
            assert tok[:3] == ["#", "col", str(k)] and tok[3] == capi.MODETABLE_KINDS[cols[k]["kind"]] and [int(t) for t in tok[4:]] == [int(cols[k][f]) for f in ("mult", "order", "l", "m", "param_index")]
            hv = header_values(blk[1:3])
            rng = np.array([float(t) for t in blk[1].split()[2:4]])
            assert np.array_equal(bits(rng), bits(h["range"][k])) and int(hv["status"]) == h["status"][k]
            assert int(hv["below"]) == h["below"][k] and int(hv["above"]) == h["above"][k]
            edge = np.array([float(x.split()[0]) for x in blk[3:3 + nb]] + [float(blk[3 + nb])])
            assert [int(x.split()[1]) for x in blk[3:3 + nb]] == list(h["counts"][k])
            assert np.array_equal(bits(edge), bits(capi.ModeTable.hist_edges(h["range"][k], nb)))
        # ---- .modes.hpd ----
        lines = open(out + ".modes.hpd").read().split("\n")
        p = want["p"]
        assert lines[0] == first and lines[2] == "# mass= 0.68,0.95" and [int(t) for t in lines[3].split()[2:]] == list(p["k"])
        assert lines[4] == "# col kind mult order l m param_index median k0.68 lo0.68 hi0.68 k0.95 lo0.95 hi0.95"
        body = [x.split() for x in lines[5:] if x]
        assert len(body) == nc
        for k, tok in enumerate(body):
            assert int(tok[0]) == k and tok[1] == capi.MODETABLE_KINDS[cols[k]["kind"]] and len(tok) == 8 + 3 * len(MASS)
            assert bits(float(tok[7])) == bits(want["med"][k])
            for m in range(len(MASS)):
                assert int(tok[8 + 3 * m]) == p["k"][m]
                assert bits(float(tok[9 + 3 * m])) == bits(p["lo"][m, k]) and bits(float(tok[10 + 3 * m])) == bits(p["hi"][m, k]), (k, m)
                assert "%.17g" % p["lo"][m, k] == tok[9 + 3 * m] and "%.17g" % p["hi"][m, k] == tok[10 + 3 * m]
        # ---- .modes.pairs ----
        lines = open(out + ".modes.pairs").read().split("\n")
        j = want[jkey]
        assert lines[0] == first and int(header_values(lines[2:3])["n_bins"]) == nb2
        body = lines[3:]
        per = 3 + nb2
        assert len([x for x in body if x]) == len(PAIRS) * per
        for q, (a, b) in enumerate(PAIRS):
            blk = body[q * per:(q + 1) * per]
            assert blk[0] == "# pair %d %d" % (a, b)
            rng = np.array([float(t) for t in blk[1].split()[2:6]])
            assert np.array_equal(bits(rng), bits(np.array([totals["min"][a], totals["max"][a], totals["min"][b], totals["max"][b]])))
            hv = header_values(blk[1:3])
            assert int(hv["status"]) == j["status"][q] and int(hv["outside"]) == j["outside"][q]
            assert int(hv["level68"]) == j["level"][0, q] and int(hv["level95"]) == j["level"][1, q]
            got = np.array([[int(t) for t in x.split()] for x in blk[3:]], dtype=np.int64)
            assert np.array_equal(got, j["counts"][q])
    # a column outside the table is refused with a message, and so is a chain too short for --modes-hpd
    r = subprocess.run(common + [str(tmp_path / "bad.txt")] + sel + ["--modes", "--modes-pairs", "0:%d" % nc], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--modes-pairs: column" in r.stderr
    r = subprocess.run(common + [str(tmp_path / "short.txt"), "--first", "4", "--last", "6", "--modes", "--modes-hpd", "0.5"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--modes-hpd needs at least 4 accepted samples" in r.stderr
