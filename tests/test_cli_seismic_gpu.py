"""chainsummary_hip --modes 0.16,0.5,0.84 --modes-indices --modes-ess on the GPU.  The stored chain: the golden local-model
inputs with one slice that spans four radial orders and three l = 1 modes written in between (the golden slices hold one
radial mode each, which the plan refuses), 50 samples from the phase driver with the oracle as evaluator, samples 4, 6, ...,
48 selected.  <output file>.modes.indices and .modes.indices.cov parse; their numbers, printed with 17 significant digits,
parse back to the bits the Python API returns for the same samples with the first of them as reference row; the .cov matrix is
symmetric with the `result` variances on its diagonal; the main output file, .modes and .modes.ess are, byte for byte, what
the same binary writes without the flag; the golden single-slice star prints the refusal and gets neither file, with 23
selected samples and with 5500 (more than the 4096 the tool reads at a time: the main file's `last=` stays that of the
passes); --modes-indices without --modes prints the usage text."""
import os
import subprocess

import numpy as np
import pytest

from summary_support import header_values, stored_chain
from support import CFG, DATA, MODEL, bits, pyorc, tool
from tamcmc_amd import capi

pytestmark = pytest.mark.gpu

L1 = ((104.30, 0.32, 1500.0), (114.70, 0.33, 1800.0), (125.30, 0.35, 1900.0))


def wide_model(tmp_path):
    """The golden .model file with one slice 94.30 ... 134.81 and the l = 1 modes of L1 after the l = 0 ones, in both lists."""
    out, slices, table = [], 0, False
    for line in open(MODEL).read().split("\n"):
        if line.startswith("* "):
            slices += 1
            if slices == 1:
                out.append("* 94.30 134.81  # Slice 1")
            continue
        tok = line.split()
        if len(tok) == 6 and tok[0] == "p" and tok[1] == "2" and not any(t.startswith("p  1") for t in out):
            out.extend("p  1  %.5f  1      1       1" % f for f, _, _ in L1)
        if len(tok) == 6 and tok[0] == "2" and not table:
            table = True
            out.extend("    1   %.5f   %.5f   %.5f     %.5f  %.5f" % (f, f - 0.4, f + 0.4, g, h) for f, g, h in L1)
        out.append(line)
    path = str(tmp_path / "wide.model")
    open(path, "w").write("\n".join(out))
    return path


def wide_chain(tmp_path):
    """summary_support.stored_chain on wide_model: (setup, rows of the selection, the tool's leading arguments, the selection)."""
    from tamcmc_amd import outputs as O
    from tamcmc_amd import sampler as S
    from tamcmc_amd.setup_io import Setup
    model, out = wide_model(tmp_path), str(tmp_path) + "/"
    s = Setup(CFG).load(model, DATA, 0)
    s.set("MALA", "Nchains", 2)
    for k, v in (("output_dir", out), ("restore_dir", out), ("output_root_name", "TF_W_"), ("Nbuffer", 50), ("file_format", "binary")):
        s.set("Outputs", k, v)
    s.set("MALA", "Nt_learn", "10, 30, 100000")
    s.apply_phase("Burn-in", 50, 1.8)
    orc = pyorc()

    def ev(P, T):
        return orc.generate_batch(s.model_case, s.plength, s.x, s.y, P, T, likelihood_p=s.likelihood_p)[:2]
    smp = S.Sampler(s.sampler_cfg(seed=5), ev, s.plength, s.inputs, s.relax, s.err, s.priors_names_switch, s.priors, s.extra_priors)
    O.run_phase(s, smp)
    root = out + "TF_W_params"
    v, _ = O.read_params_bin(root, 0)
    rows = np.tile(s.inputs, (23, 1))
    rows[:, s.index_to_relax] = v[4::2]
    return s, rows, [tool(), CFG, model, DATA, root], ["--thin", "2", "--first", "4", "--block", "7"]


def same_file(a, b):
    return open(a, "rb").read().replace(a.encode(), b"@") == open(b, "rb").read().replace(b.encode(), b"@")


def test_command_line(accel_mod, tmp_path):
    s, rows, common, sel = wide_chain(tmp_path)
    assert list(s.plength[2:6]) == [4, 3, 4, 3]
    Q = [0.16, 0.5, 0.84]
    with accel_mod.Accel(s.model_case, s.plength, s.x, s.y, sigma_y=s.sigma_y, likelihood_case=s.likelihood_case,
                         likelihood_p=s.likelihood_p) as acc, capi.ModeTable(acc, len(rows)) as mt:
        st = mt.derive(rows)[1]
        assert st[0] == 0                                   # the first selected sample is the reference row
        info = mt.enable_indices(rows[0])
        cols = mt.columns()
        assert np.all(mt.push(rows) == 0)
        res, q, e = mt.result(), mt.quantiles(Q), mt.ess(0)
        nb, ni = info["n_base_cols"], info["n_index_cols"]
        ratio = np.flatnonzero(cols["kind"] >= len(capi.MODETABLE_KINDS) + capi.SEISMIC_KINDS.index("r02")).astype(np.int32)
        cov = mt.cov(ratio)
    assert info["n_radial"] == 4 and ni > 10 and ratio.size >= 2
    plain = str(tmp_path / "plain.txt")
    r = subprocess.run(common + [plain] + sel + ["--modes", "0.16,0.5,0.84", "--modes-ess"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(plain + ".modes") and not os.path.exists(plain + ".modes.indices") and not os.path.exists(plain + ".modes.indices.cov")
    r = subprocess.run(common + [str(tmp_path / "none.txt")] + sel + ["--modes-indices"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr and "--modes-indices needs --modes" in r.stderr
    assert not os.path.exists(str(tmp_path / "none.txt"))
    out = str(tmp_path / "ind.txt")
    r = subprocess.run(common + [out] + sel + ["--modes", "0.16,0.5,0.84", "--modes-indices", "--modes-ess"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert same_file(out, plain) and same_file(out + ".modes", plain + ".modes") and same_file(out + ".modes.ess", plain + ".modes.ess")
    lines = open(out + ".modes.indices").read().split("\n")
    head = header_values(line for line in lines if line.startswith("#") and "=" in line)
    assert lines[0].startswith("# chainsummary_hip (") and lines[0] == open(out + ".modes").readline().rstrip("\n")
    assert lines[1] == "# quantiles= 0.16,0.5,0.84" and lines[3] == "# col kind l n mean sd q0.16 q0.5 q0.84 ess tau mcse rhat cut"
    for k in ("n_base_cols", "n_index_cols", "n_radial", "n_unassigned", "n_base"):
        assert int(head[k]) == info[k], k
    assert int(head["n_used"]) == res["n_used"] == 23 and int(head["n_rejected"]) == 0
    assert bits(float(head["dnu_ref"])) == bits(info["dnu_ref"]) and bits(float(head["eps_ref"])) == bits(info["eps_ref"])
    body = [line.split() for line in lines[4:] if line]
    assert len(body) == ni
    for j, tok in enumerate(body):
        k, c = nb + j, cols[nb + j]
        assert int(tok[0]) == k and tok[1] == capi.ModeTable.KINDS[c["kind"]] and (int(tok[2]), int(tok[3])) == (c["l"], c["order"]) and len(tok) == 14
        got = np.array([float(t) for t in tok[4:13]])
        ref = np.array([res["mean"][k], res["sd"][k]] + [q["values"][i, k] for i in range(3)] + [e[name][k] for name in ("ess", "tau", "mcse", "rhat")])
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(bits(got[~np.isnan(got)]), bits(ref[~np.isnan(ref)])), (k, got, ref)
        assert int(tok[13]) == e["cut"][k]
    clines = open(out + ".modes.indices.cov").read().split("\n")
    assert clines[0] == lines[0] and clines[2] == "# cols = " + " ".join(str(int(k)) for k in ratio)
    names = clines[3].split()[3:]
    assert clines[3].startswith("# rows = ") and names == ["%s_n%d" % (capi.ModeTable.KINDS[cols["kind"][k]], cols["order"][k]) for k in ratio]
    M = np.array([[float(t) for t in line.split()] for line in clines[4:] if line])
    assert M.shape == (ratio.size, ratio.size) and np.array_equal(bits(M), bits(cov)) and np.array_equal(bits(M), bits(M.T))
    # the diagonal against result's variance: Welford's M2 against the sum of squared centred values, both of n = 23 terms; the
    # running mean carries 2^-52 |mean| per step, which enters a deviation relative to sd
    var, amp = res["sd"][ratio] ** 2, 1.0 + np.abs(res["mean"][ratio]) / res["sd"][ratio]
    assert np.all(var > 0) and np.all(np.abs(np.diag(M) - var) <= 8 * 2.0 ** -52 * 23 * amp * var)
    # the golden star, one radial mode in its slice: the refusal, neither file, everything else as without the flag
    s1, root1, v1, rows1, common1, sel1 = stored_chain(tmp_path)
    a, b = str(tmp_path / "g_plain.txt"), str(tmp_path / "g_ind.txt")
    r = subprocess.run(common1 + [a] + sel1 + ["--modes"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run(common1 + [b] + sel1 + ["--modes", "--modes-indices"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--modes-indices refused" in r.stderr and "radial" in r.stderr, r.stdout + r.stderr
    assert same_file(a, b) and same_file(a + ".modes", b + ".modes") and not os.path.exists(b + ".modes.indices") and not os.path.exists(b + ".modes.indices.cov")
    # the same star with more samples than one pass of the tool reads at a time (4096): the rows of the file 110 times over.  The
    # search for the reference row stops at the first sample and must leave the main file's `last=` where the passes put it.
    binf = root1 + "_chain-0.bin"
    raw = open(binf, "rb").read()
    open(binf, "wb").write(raw * 110)
    a, b = str(tmp_path / "long_plain.txt"), str(tmp_path / "long_ind.txt")
    r = subprocess.run(common1 + [a, "--modes"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run(common1 + [b, "--modes", "--modes-indices"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--modes-indices refused" in r.stderr, r.stdout + r.stderr
    head = header_values(line for line in open(b).read().split("\n")[:4] if line.startswith("#") and "=" in line)
    assert int(head["samples_in_file"]) == 5500 and int(head["last"]) == 5499 and int(head["n_used"]) + int(head["n_rejected"]) == 5500
    assert same_file(a, b) and same_file(a + ".modes", b + ".modes") and not os.path.exists(b + ".modes.indices") and not os.path.exists(b + ".modes.indices.cov")
