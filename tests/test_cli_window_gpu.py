"""bin/chainsummary_hip --window on the GPU: the 23-sample chain of tests/test_summary_gpu.py::test_command_line on the
golden local-model inputs.  --window 7,3 writes <output file>.windows, whose header and rows are the numbers
Summary(..., window=(7, 3)).window_result() gives to the 12 printed digits; the output file itself is, byte for byte, what
the same binary writes without the flag, with and without --predictive."""
import os
import subprocess

import numpy as np
import pytest

from tamcmc_amd import capi
from test_summary_gpu import CFG, G, ROOT, pyorc

pytestmark = pytest.mark.gpu


def test_command_line(accel_mod, tmp_path):
    from tamcmc_amd import outputs as O
    from tamcmc_amd import sampler as S
    from tamcmc_amd.setup_io import Setup
    exe = os.path.join(ROOT, "bin", "chainsummary_hip")
    model, data = os.path.join(G, "TF_3443483_local-v3.model"), os.path.join(G, "TF_3443483_local-v3.data")
    out = str(tmp_path) + "/"
    s = Setup(CFG).load(model, data, 0)
    s.set("MALA", "Nchains", 2)
    for k, v in (("output_dir", out), ("restore_dir", out), ("output_root_name", "TF_A_"), ("Nbuffer", 50), ("file_format", "binary")):
        s.set("Outputs", k, v)
    s.set("MALA", "Nt_learn", "10, 30, 100000")
    s.apply_phase("Burn-in", 50, 1.8)
    orc = pyorc()

    def ev(P, T):
        return orc.generate_batch(s.model_case, s.plength, s.x, s.y, P, T, likelihood_p=s.likelihood_p)[:2]
    smp = S.Sampler(s.sampler_cfg(seed=5), ev, s.plength, s.inputs, s.relax, s.err, s.priors_names_switch, s.priors, s.extra_priors)
    O.run_phase(s, smp)
    root = out + "TF_A_params"
    v, _ = O.read_params_bin(root, 0)
    common = [exe, CFG, model, data, root]
    sel = ["--thin", "2", "--first", "4", "--block", "7"]
    rows = np.tile(s.inputs, (23, 1))
    rows[:, s.index_to_relax] = v[4::2]
    with accel_mod.Accel(s.model_case, s.plength, s.x, s.y, sigma_y=s.sigma_y, likelihood_case=s.likelihood_case,
                         likelihood_p=s.likelihood_p) as acc:
        with capi.Summary(acc, window=(7, 3)) as sm:
            _, st = sm.push(rows)
            d = sm.window_result()
    assert np.all(st == 0) and d["n_used"] == 23 and d["n_windows"] == 1 + -(-(s.Nx - 3) // 7)
    f12 = lambda a: np.array([float("%.12g" % t) for t in np.atleast_1d(a)])       # noqa: E731
    for extra in ([], ["--predictive"]):
        plain, table = str(tmp_path / f"plain{len(extra)}.txt"), str(tmp_path / f"win{len(extra)}.txt")
        for path, flag in ((plain, []), (table, ["--window", "7,3"])):
            r = subprocess.run(common + [path] + sel + extra + flag, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout + r.stderr
        assert open(table, "rb").read() == open(plain, "rb").read(), "the output file changed with --window"
        assert not os.path.exists(plain + ".windows")
        lines = open(table + ".windows").read().split("\n")
        head = [line for line in lines if line.startswith("#")]
        assert lines[:len(head)] == head and lines[-1] == "" and len(lines) == len(head) + d["n_windows"] + 1
        assert head[0].startswith("# chainsummary_hip (") and head[-1] == "# w first_bin last_bin x_first x_last pit log_cdf log_sf mean_resid"
        val = {}
        for line in head[1:-2]:
            tok = line[1:].split()
            val.update({a[:-1]: b for a, b in zip(tok, tok[1:]) if a.endswith("=")})
        for key in ("W", "first", "n_windows", "n_used", "n_rejected", "win_min_log_sf", "win_min_log_cdf"):
            assert int(val[key]) == d[key], key
        assert (d["W"], d["first"]) == (7, 3)
        for key in ("ks_D", "min_log_sf", "min_log_cdf"):
            assert val[key] == "%.12g" % d[key], key
        assert head[-2].startswith("# pit_hist=")
        hist = [int(c) for c in head[-2].split("=")[1].split()]
        assert hist == list(d["pit_hist"]) and sum(hist) == d["n_windows"]
        t = np.loadtxt(table + ".windows")
        assert t.shape == (d["n_windows"], 9)
        assert np.array_equal(t[:, 0], np.arange(d["n_windows"])) and np.array_equal(t[:, 1], d["first_bin"]) and np.array_equal(t[:, 2], d["last_bin"])
        assert np.array_equal(t[:, 3], f12(s.x[d["first_bin"]])) and np.array_equal(t[:, 4], f12(s.x[d["last_bin"]]))
        for j, key in enumerate(("pit", "log_cdf", "log_sf", "mean_resid")):
            assert np.array_equal(t[:, 5 + j], f12(d[key])), key
