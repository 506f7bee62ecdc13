"""The three kernels of tamcmc_modetable.hip cross-compiled for gfx950 (make resource-usage-modetable): none uses scratch or
spills a vector register, and each stays within 64 KiB of LDS per workgroup -- the derive kernel holds a multiplet's whole
record (TmMultFull) in registers, as the setup kernel does, and its static LDS is the chain record alone (the params row is
dynamic LDS, at most 60 KiB by tamcmc_modetable_create); the quantile kernel's LDS is its eight 256-cell histograms.  The
scalar-register spills of each kernel are printed (they go to vector registers, not to memory)."""
from support import kernel_usage, needs_hipcc


@needs_hipcc
def test_kernel_resources():
    usage = kernel_usage("resource-usage-modetable")           # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == 3, sorted(usage)
    kinds = {k: [s for s in ("derive_kernel", "fold_kernel", "quantile_kernel") if s in k] for k in usage}
    assert sorted(v[0] for v in kinds.values()) == ["derive_kernel", "fold_kernel", "quantile_kernel"], sorted(usage)
    for k, (scratch, sspill, vspill, lds) in usage.items():
        print(f"{kinds[k][0]}: SGPR spills {sspill}, LDS {lds} bytes")
        assert scratch == 0 and vspill == 0, (k, scratch, vspill)
        assert lds <= 64 * 1024, (k, lds)
        if "fold_kernel" in k:
            assert lds == 0
        if "quantile_kernel" in k:
            assert lds == 8 * 256 * 4 + 3 * 8 * 8
