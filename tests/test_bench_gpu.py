"""bench.py's plain run: the contract line holds the headline keys and only those legs a plain run needs, and
`--dump-outputs` writes what the last timed step computed -- the same arrays from run to run, and the oracle's logL and
analytic gradient on the bench's own inputs (tolerances of tests/gradcheck.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gradcheck
from tamcmc_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, CHAINS, STEPS = 20000, 8, 5


def run_bench(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "2",
                        "--nx", str(NX), "--chains", str(CHAINS), "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {n: np.load(os.path.join(out_dir, n + ".npy")) for n in ("logL", "grad", "status")}


def test_plain_run_line_and_dumped_outputs(accel_mod, orc, tmp_path):
    line, out = run_bench(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == STEPS and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert abs(line["value"] - CHAINS * 1e3 / line["ms_per_step"]) <= 1e-2 * line["value"]     # ms_per_step has 4 decimals
    for k in ("roofline", "logL_only", "host_path", "ensemble", "sampler", "sampler_sharded", "cpu_baseline"):
        assert k not in line, k

    w = synth.workload_c2(model_case=2, Nx=NX)
    P, T = synth.chain_params(w, CHAINS), synth.temperatures(CHAINS)
    nvars = w["index_to_relax"].size
    assert out["logL"].shape == (CHAINS,) and out["grad"].shape == (CHAINS, nvars) and out["status"].shape == (CHAINS,)
    assert all(a.dtype == np.float64 for a in out.values())
    assert np.all(out["status"] == 0)

    # the bench's inputs, rebuilt the way it builds them
    with accel_mod.Accel(2, w["plength"], w["x"], np.ones(NX)) as acc:
        m_true, st = acc.model_explicit(w["params_true"])
    assert st == 0
    y = synth.make_spectrum(m_true)
    ref, rst = orc.generate_batch(2, w["plength"], w["x"], y, P, T)
    assert np.all(rst == 0)
    assert np.max(np.abs(out["logL"] - ref) / np.abs(ref)) <= 1e-10
    gref, gabs, _, gst = orc.grad_analytic(2, w["plength"], w["x"], y, P, T, w["index_to_relax"])
    assert np.all(gst == 0)
    gradcheck.assert_grad_entrywise(out["grad"], gref, gabs, "bench --dump-outputs")

    # same arguments, same inputs: a second run writes the same arrays
    _, again = run_bench(tmp_path / "b")
    for n in out:
        assert np.array_equal(out[n], again[n]), n
