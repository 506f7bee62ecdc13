"""The three kernels of tamcmc_modediag.hip cross-compiled for gfx950 (make resource-usage-modediag): none uses scratch or
spills a vector register, and each stays within 64 KiB of LDS per workgroup -- the lag kernel's tile and halo of 1024 doubles
each (16 KiB), the covariance kernel's two strips of 64 rows of 34 doubles (34 KiB), the finish kernel none.  The
scalar-register spills of each kernel are printed (they go to vector registers, not to memory)."""
from support import kernel_usage, needs_hipcc


@needs_hipcc
def test_kernel_resources():
    usage = kernel_usage("resource-usage-modediag")            # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == 3, sorted(usage)
    kinds = {k: [s for s in ("lag_kernel", "finish_kernel", "cov_kernel") if s in k] for k in usage}
    assert sorted(v[0] for v in kinds.values()) == ["cov_kernel", "finish_kernel", "lag_kernel"], sorted(usage)
    for k, (scratch, sspill, vspill, lds) in usage.items():
        print(f"{kinds[k][0]}: SGPR spills {sspill}, LDS {lds} bytes")
        assert "modediag" in k
        assert scratch == 0 and vspill == 0, (k, scratch, vspill)
        assert lds <= 64 * 1024, (k, lds)
        if "lag_kernel" in k:
            assert lds == (1024 + 1024) * 8
        if "finish_kernel" in k:
            assert lds == 0
        if "cov_kernel" in k:
            assert lds == 2 * 64 * 34 * 8
