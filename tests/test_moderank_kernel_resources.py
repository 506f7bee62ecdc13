"""The three kernels of tamcmc_moderank.hip cross-compiled for gfx950 (make resource-usage-moderank): none uses scratch or
spills a vector register; the sort kernel's LDS is the tile of TM_MR_TILE = 8192 keys the header states (TM_MR_LDS_BYTES =
65 536 bytes, within the 160 KiB a workgroup may declare), the transform and mean kernels use none.  The scalar-register
spills of each kernel are printed (they go to vector registers, not to memory)."""
import os
import re

from support import kernel_usage, needs_hipcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@needs_hipcc
def test_kernel_resources():
    hdr = open(os.path.join(ROOT, "tamcmc-c-_amd", "csrc", "tamcmc_moderank.h")).read()
    tile = int(re.search(r"#define TM_MR_TILE (\d+)", hdr).group(1))
    assert re.search(r"#define TM_MR_LDS_BYTES \(TM_MR_TILE \* 8\)", hdr) and "65 536 bytes" in hdr
    usage = kernel_usage("resource-usage-moderank")            # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == 3, sorted(usage)
    kinds = {k: [s for s in ("sort_kernel", "transform_kernel", "mean_kernel") if s in k] for k in usage}
    assert sorted(v[0] for v in kinds.values()) == ["mean_kernel", "sort_kernel", "transform_kernel"], sorted(usage)
    for k, (scratch, sspill, vspill, lds) in usage.items():
        print(f"{kinds[k][0]}: SGPR spills {sspill}, LDS {lds} bytes")
        assert "moderank" in k
        assert scratch == 0 and vspill == 0, (k, scratch, vspill)
        assert lds <= 160 * 1024, (k, lds)
        assert lds == (tile * 8 if "sort_kernel" in k else 0), (k, lds)
    assert tile * 8 == 65536
