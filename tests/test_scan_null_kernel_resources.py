"""Resources of the scan null's kernels (tamcmc_scan_null.hip), cross-compiled for gfx950 (make resource-usage-scan_null):
exactly three kernels -- extremes, combine, variates -- none of which uses scratch or spills a register (the per-width running
extremes of a lane are indexed by unrolled loops and stay in registers), and LDS only in the extremes kernel: the tile's
variates with their halo and the waves' partial extremes, TM_NULL_LDS_BYTES of tamcmc_scan_null.h to the byte."""
import os
import re

from support import CSRC, kernel_usage, needs_hipcc

KERNELS = ("tamcmc_scan_null_extremes_kernel", "tamcmc_scan_null_combine_kernel", "tamcmc_scan_null_variates_kernel")


def stated_lds():
    """TM_NULL_LDS_BYTES worked out from the defines of the two headers."""
    scan = open(os.path.join(CSRC, "tamcmc_scan.h")).read()
    win = open(os.path.join(CSRC, "tamcmc_window.h")).read()
    null = open(os.path.join(CSRC, "tamcmc_scan_null.h")).read()
    tile = int(re.search(r"#define TM_SCAN_TILE (\d+)", scan).group(1))
    widths = int(re.search(r"#define TM_SCAN_MAX_WIDTHS (\d+)", scan).group(1))
    bins = int(re.search(r"#define TM_WIN_MAX_BINS (\d+)", win).group(1))
    threads = int(re.search(r"#define TM_NULL_THREADS (\d+)", null).group(1))
    assert "#define TM_NULL_LDS_BYTES ((TM_SCAN_LDS_DOUBLES * 8 + 15) / 16 * 16 + TM_NULL_WAVES * TM_SCAN_MAX_WIDTHS * 2 * 12)" in null
    assert "#define TM_SCAN_LDS_DOUBLES (TM_SCAN_TILE + TM_WIN_MAX_BINS - 1)" in scan and "#define TM_NULL_WAVES (TM_NULL_THREADS / 64)" in null
    return ((tile + bins - 1) * 8 + 15) // 16 * 16 + threads // 64 * widths * 2 * 12


@needs_hipcc
def test_scan_null_kernel_resources():
    usage = kernel_usage("resource-usage-scan_null")        # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == len(KERNELS) and all(any(k in name for name in usage) for k in KERNELS), sorted(usage)
    lds = stated_lds()
    assert lds == 21248
    for name, v in usage.items():
        assert v[:3] == (0, 0, 0), (name, v)
        assert v[3] == (lds if KERNELS[0] in name else 0), (name, v)
