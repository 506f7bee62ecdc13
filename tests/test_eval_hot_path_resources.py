"""Scalar spills and registers of the four eval kernels, from the metadata of their cross-compiled gfx950 assembly
(make eval-asm).

The common-case kernels (GEN = false: tamcmc_eval_kernel<true,false> for the gradient, <false,false> for the likelihood)
walk polynomial cells in loops of their own (tamcmc_eval_body.h).  Before that split the exp fallback shared the group
loop with the polynomial code behind a per-cell branch: its scalars were live through the loop, 40 / 44 SGPRs were
spilled and reloaded inside it, and the accumulators were copied where the two variants joined.

What is pinned, and what it means:
  * .sgpr_spill_count of the build at hand.  It is a STATIC count over the whole kernel, cold loops included -- the figure
    that matters at run time, the reloads inside the polynomial pair loop, is in profiles/README.md ("hot-path audit");
  * .vgpr_count not above the values before the split (117 / 69), no spilled VGPR, no scratch.

Both common-case kernels now spill fewer scalars than before the split (38 < 40, 39 < 44).  What is still spilled is
spilled around the loops, not inside them: 16 of the gradient kernel's 38 are one block of kernel arguments that only
pass 2 reads, written once in the prologue, and its pair loop holds no v_readlane where the loop before the split
reloaded 16 SGPRs per multiplet.  Two things the cold loops would otherwise cost are kept out by an empty asm each
(tamcmc_eval_body.h): the `h < nh` masks of the fallback and the lane masks of the cold loop's noise flush, which the
compiler hoisted in front of that loop and spilled across it (43 SGPRs without them)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tamcmc-c-_amd", "csrc")

# (GRAD, GEN) -> pinned .sgpr_spill_count / ceiling of .vgpr_count.  Build: hipcc of ROCm 7.2 (AMD clang 22), -O3, gfx950, the
# flags of `make eval-asm`; the VGPR ceilings of the common-case kernels are the counts before the cell-kind split.
SGPR_SPILLS = {(True, False): 38, (False, False): 39, (True, True): 68, (False, True): 54}
VGPR_MAX = {(True, False): 117, (False, False): 69, (True, True): 128, (False, True): 72}
SGPR_SPILLS_BEFORE = {(True, False): 40, (False, False): 44}


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("evalasm")
    r = subprocess.run(["make", "-s", "-C", CSRC, "eval-asm", f"ASMDIR={d}"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    asm = (d / "tamcmc_eval.s").read_text()
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", asm)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_Z18tamcmc_eval_kernelILb([01])ELb([01])E", name)
        if not m:
            continue
        field = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))
        out[(m.group(1) == "1", m.group(2) == "1")] = dict(sgpr_spills=field("sgpr_spill_count"), vgprs=field("vgpr_count"),
                                                         vgpr_spills=field("vgpr_spill_count"),
                                                         scratch=field("private_segment_fixed_size"))
    assert sorted(out) == sorted(SGPR_SPILLS), sorted(out)
    return out


@pytest.mark.parametrize("grad,gen", sorted(SGPR_SPILLS), ids=lambda v: str(int(v)))
def test_registers_of_the_eval_kernels(metadata, grad, gen):
    m = metadata[(grad, gen)]
    print(f"\ntamcmc_eval_kernel<{int(grad)},{int(gen)}>: {m}")
    assert m["vgprs"] <= VGPR_MAX[(grad, gen)], m
    assert m["vgpr_spills"] == 0 and m["scratch"] == 0, m
    assert m["sgpr_spills"] <= SGPR_SPILLS[(grad, gen)], m


@pytest.mark.parametrize("grad", [True, False], ids=["gradient", "likelihood"])
def test_common_case_kernels_spill_fewer_scalars_than_before_the_split(metadata, grad):
    m = metadata[(grad, False)]
    print(f"\ntamcmc_eval_kernel<{int(grad)},0>: {m['sgpr_spills']} spilled SGPRs, before the split {SGPR_SPILLS_BEFORE[(grad, False)]}")
    assert m["sgpr_spills"] < SGPR_SPILLS_BEFORE[(grad, False)], m
