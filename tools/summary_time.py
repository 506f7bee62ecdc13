#!/usr/bin/env python
"""Times the posterior summary (tamcmc_amd.Summary) on C2's grid: Nx = 1e5 bins, model id 2, S rows of synth.chain_params.

Prints one JSON line:
  a_summary_s_per_1000      seconds per 1000 samples through Summary.push (host pointers, blocks of --block)
  b_host_route_s_per_1000   the same work without the summary object: eval_batch with every chain in model_rows in blocks
                            of 64, S x Nx doubles through host memory, and the same recurrences in numpy, sample by sample
                            (timed on --samples-b rows: it is slow)
  c_fold_*                  the fold kernel alone, from HIP events around every launch: time per block, bytes per second
                            (the block's rows read once + the running state read and written) and that rate over the
                            6.29 TB/s measured copy ceiling of the MI355X
  d_quantile_*              quantile mode (Summary.quantiles_*) at --quantiles quantiles and --qbits bits per pass, after leg
                            (a)'s fold pass: seconds per pass per 1000 samples through Summary.push (the step included), the
                            histogram kernel alone from the same HIP-event hooks, and the number of passes to exactness
  e_loo_*                   LOO mode (Summary.loo_*) after a fold pass of the same rows: the tail pass in seconds per 1000
                            samples through Summary.push, the tail kernel alone per block and the finalize kernel alone,
                            once, from the same HIP-event hooks, M, and the device memory the mode allocates
  f_predictive_*            with --predictive (and --like-p p, default 1): in one run, the fold pass through Summary.push with
                            the predictive check off and on (two summary objects on one context, alternating, seconds per
                            1000 samples), and from a profiled pass of the second object the fold kernel alone
                            (Summary.kernel_time) beside the predictive kernel alone (Summary.predictive_kernel_time) and
                            the eval launches of the same blocks (Accel.kernel_time).  Only this leg runs.
  g_window_*                with --window W (and --like-p p, default 1; p W <= 512): the same for the windowed check -- the fold
                            pass with the check off and on, alternating in one run, and from a profiled pass the fold kernel
                            alone beside the three window kernels together (Summary.window_kernel_time) and the eval launches.
                            Only this leg runs.
  h_ess_*                   with --ess L (0: the library's default lag limit): the fold pass and the ESS pass of the same rows
                            through Summary.push, alternating in one run (seconds per 1000 samples), and from profiled passes the
                            fold kernel alone beside the ESS kernels alone (centre and lag kernels of every block,
                            Summary.kernel_time in ESS mode) and the eval launches, the finish kernel, ess_result on the host
                            clock, and the device memory the mode allocates.  Only this leg runs.
  i_scan_*                  with --scan W0[,W1,...] (and --like-p p, default 1; p times the largest width <= 512): the same as
                            (g) for the sliding-window scan -- the fold pass with the scan off and on, alternating in one run,
                            and from a profiled pass the fold kernel alone beside all scan kernels of a block together
                            (Summary.scan_kernel_time) and the eval launches; per width the minima found and the number of
                            regions below the default line.  Only this leg runs.
  j_scan_null_*             with --scan-null R (and --scan W0[,W1,...], default 10,20,40; --like-p p; --nx): the Monte-Carlo null of
                            the scan (tamcmc_amd.ScanNull), no chain and no context: R replicates per run, --warmup + --steps
                            runs appended to one object -- wall seconds per replicate through ScanNull.run (the copy back and the
                            host's tail functions included) and the two kernels alone from HIP events around every chunk; the
                            joint and the per-width 1 % line of the excess side beside the default line.  Only this leg runs.
  k_bandess_*               with --band-ess L (0: the library's default lag limit; --quantiles K thresholds, default 3): after a fold
                            pass and the exact selection of K quantiles, the band ESS pass of the same rows through Summary.push
                            beside the fold pass, alternating in one run (seconds per 1000 samples), and from profiled passes the
                            fold kernel alone beside the band kernels alone (pack and lag kernels of every block,
                            Summary.kernel_time in the mode) and the eval launches, the finish kernels (one per threshold),
                            bandess_result on the host clock, and the device memory the mode allocates.  Only this leg runs.
  l_loo_pit_*               with --loo-pit (and --like-p p, default 1): after a fold pass, in one run, the LOO tail pass and the
                            LOO-PIT pass of the same rows through Summary.push, alternating (seconds per 1000 samples), and from
                            profiled passes in the same session the PIT kernel alone (Summary.loo_pit_kernel_time) beside the tail
                            kernel alone, the predictive kernel alone (a second object with the check on) and the eval launches,
                            loo_pit_begin on the host clock and its prepare kernel alone, and the device memory the sub-mode
                            allocates.  Only this leg runs.
  m_wloo_*                  with --loo-window W (and --like-p p, default 1; p W <= 512): after a fold pass, in one session, the
                            window-LOO pass and its PIT pass of the same rows through Summary.push (seconds per 1000 samples),
                            and from profiled passes the mode's kernels alone -- the sums and tail kernels of every block
                            (Summary.kernel_time in the mode), the sums, tails and PIT kernels of every block of the third pass
                            (Summary.wloo_pit_kernel_time) -- beside the per-bin LOO tail kernel and the per-bin LOO-PIT kernel
                            of the same rows, the finalize and prepare kernels over the windows, and the device memory the mode
                            and its sub-mode allocate.  Only this leg runs.
  n_modetable_*             with --modes: the posterior mode table (tamcmc_amd.ModeTable) of the same rows, no spectrum involved:
                            ModeTable.push on the host clock (seconds per 1000 samples, staging and the per-block status
                            round trip included), the derive and fold kernels alone from the object's HIP events
                            (ModeTable.kernel_time: microseconds per sample, launches), the quantile call for three
                            probabilities on the host clock (--quantiles sets their number), the number of columns and the
                            device memory of the table.  Only this leg runs.
  p_moderank_*              with --modes and --modes-rank L: the rank-normalised diagnostics of that table's columns -- the summed
                            kernel time of a rank_diag call (sort twice, transform, mean, lag, finish per chunk), the call's wall
                            time, and the same statements on one host thread (tools/moderank_host_time.cpp, std::sort)
  r_modepdf_*               with --modes and --modes-pdf: the marginal posteriors of that table's columns -- the hist call at 50 classes
                            on all columns and on the integer window-edge columns alone, the hpd call at masses 0.68 and 0.95 and at
                            mass 1 (one window start: the sort launch by itself), the hist2d call over the
                            (width, height) pair of every multiplet at 32 classes: kernel time and wall time of each, beside the
                            table's own derive and fold kernels and the same statements on one host thread
                            (tools/modepdf_host_time.cpp, std::sort)
  s_compare_*               with --compare K,R (and --nx N): the comparison of K fits (tamcmc_amd.Compare) over N units of pseudo-random
                            pointwise values, no chain and no context: R replicates of the Bayesian bootstrap after a warm-up
                            call -- wall seconds and, from HIP events around every chunk, kernel seconds per replicate, and
                            the variates per second (R N' / kernel time) -- then the stacking fit (tol 1e-8, at most 2000
                            iterations) with and without the table of P: iterations, wall time, kernel time in total and per
                            iteration; beside them the header's serial statements on one host thread
                            (tools/compare_host_time.cpp, built with g++ when the leg runs).  Only this leg runs.
  o_modediag_*              with --modes and --modes-ess L and / or --modes-cov: the diagnostics of that table's columns
                            (ModeTable.ess / ModeTable.cov) on the rows it holds: per call the kernels alone from the object's HIP
                            events (ModeTable.diag_kernel_time: lag and finish kernels of an ess call together, the covariance
                            kernel of a cov call) and the call on the host clock; beside them the table's own derive and fold
                            kernels of the same rows, and the same lag products and sums of products by the header's serial
                            functions on one host thread (tools/modediag_host_time.cpp, built with g++ when the leg runs) with
                            the ratios.  Only this leg runs.
  q_seismic_*               with --modes and --modes-indices: the seismic indices (ModeTable.enable_indices, reference row
                            params_true).  The same rows through a table without and a table with the indices: push on the host
                            clock, the derive and fold kernels (ModeTable.kernel_time) and the indices kernel alone
                            (ModeTable.seismic_kernel_time) in microseconds per sample, and the quantile (three
                            probabilities), ess and rank_diag calls of either table on the host clock.  Only this leg runs.
Every timed shape is warmed up first (--warmup pushes); host clocks stop after calls that end in a device synchronise.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import tamcmc_amd  # noqa: E402
from tamcmc_amd import synth  # noqa: E402

COPY_CEILING = 6.29e12


def host_fold(acc, P, y, like_p=1.0, block=64):
    """The route without the summary object: model rows to the host, Welford + running-maximum log-sum-exp in numpy."""
    nx = y.size
    n = 0
    mean, M2, ml, M2l = np.zeros(nx), np.zeros(nx), np.zeros(nx), np.zeros(nx)
    mn = mx = a = r = None
    for k in range(0, len(P), block):
        Pb = P[k:k + block]
        _, st, rows = acc.eval_batch(Pb, np.ones(len(Pb)), model_rows=np.arange(len(Pb)))
        for s in range(len(Pb)):
            if st[s] != 0:
                continue
            n += 1
            v = rows[s]
            l = -like_p * (y / v + np.log(v))
            d = v - mean; mean += d / n; M2 += d * (v - mean)
            d = l - ml; ml += d / n; M2l += d * (l - ml)
            if n == 1:
                mn, mx, a, r = v.copy(), v.copy(), l.copy(), np.ones(nx)
            else:
                np.minimum(mn, v, out=mn); np.maximum(mx, v, out=mx)
                up = l > a
                r = np.where(up, r * np.exp(np.minimum(a - l, 0.0)) + 1.0, r + np.exp(np.minimum(l - a, 0.0)))
                a = np.where(up, l, a)
    return dict(mean_M=mean, var_M=M2 / (n - 1), lppd=a + np.log(r / n), var_l=M2l / (n - 1), n_used=n)


def predictive_leg(a, w, y, P):
    """(f) the fold pass with the predictive check off and on, and the kernels' own times."""
    out = dict(f_predictive_like_p=a.like_p)
    with tamcmc_amd.Accel(2, w["plength"], w["x"], y, likelihood_p=float(a.like_p)) as acc:
        with tamcmc_amd.Summary(acc, a.block) as s0, tamcmc_amd.Summary(acc, a.block, predictive=True) as s1:
            times = {0: [], 1: []}
            for k in range(a.warmup + a.steps):
                for on, s in ((0, s0), (1, s1)):
                    s.reset()
                    acc.synchronize()
                    t0 = time.perf_counter()
                    s.push(P)                               # synchronous: results are on the host on return
                    if k >= a.warmup:
                        times[on].append(time.perf_counter() - t0)
            for on, key in ((0, "off"), (1, "on")):
                out[f"f_predictive_{key}_s_per_1000"] = float(np.median(times[on])) * 1000.0 / a.samples
                out[f"f_predictive_{key}_spread"] = [float(min(times[on])) * 1000.0 / a.samples, float(max(times[on])) * 1000.0 / a.samples]
            s1.reset()
            s1.profile(True)
            acc.profile(True)
            s1.push(P)
            fold_ms, launches = s1.kernel_time()
            pred_ms, pred_launches = s1.predictive_kernel_time()
            eval_ms, eval_launches = acc.kernel_time()
            acc.profile(False)
            s1.profile(False)
            r = s1.predictive_result()
            out.update(f_predictive_launches=pred_launches, f_fold_us_per_block=fold_ms * 1e3 / launches,
                       f_predictive_us_per_block=pred_ms * 1e3 / pred_launches, f_eval_us_per_block=eval_ms * 1e3 / max(eval_launches, 1),
                       f_fold_kernel_s_per_1000=fold_ms * 1e-3 * 1000.0 / a.samples,
                       f_predictive_kernel_s_per_1000=pred_ms * 1e-3 * 1000.0 / a.samples,
                       f_eval_kernel_s_per_1000=eval_ms * 1e-3 * 1000.0 / a.samples,
                       f_predictive_ks_D=r["ks_D"], f_predictive_min_log_sf=r["min_log_sf"], n_used=r["n_used"])
    return out


def window_leg(a, w, y, P):
    """(g) the fold pass with the windowed check off and on, and the kernels' own times."""
    out = dict(g_window_W=a.window, g_window_like_p=a.like_p)
    with tamcmc_amd.Accel(2, w["plength"], w["x"], y, likelihood_p=float(a.like_p)) as acc:
        with tamcmc_amd.Summary(acc, a.block) as s0, tamcmc_amd.Summary(acc, a.block, window=a.window) as s1:
            times = {0: [], 1: []}
            for k in range(a.warmup + a.steps):
                for on, s in ((0, s0), (1, s1)):
                    s.reset()
                    acc.synchronize()
                    t0 = time.perf_counter()
                    s.push(P)                               # synchronous: results are on the host on return
                    if k >= a.warmup:
                        times[on].append(time.perf_counter() - t0)
            for on, key in ((0, "off"), (1, "on")):
                out[f"g_window_{key}_s_per_1000"] = float(np.median(times[on])) * 1000.0 / a.samples
                out[f"g_window_{key}_spread"] = [float(min(times[on])) * 1000.0 / a.samples, float(max(times[on])) * 1000.0 / a.samples]
            s1.reset()
            s1.profile(True)
            acc.profile(True)
            s1.push(P)
            fold_ms, launches = s1.kernel_time()
            win_ms, win_blocks = s1.window_kernel_time()
            eval_ms, eval_launches = acc.kernel_time()
            acc.profile(False)
            s1.profile(False)
            r = s1.window_result()
            out.update(g_window_blocks=win_blocks, g_window_n_windows=r["n_windows"], g_fold_us_per_block=fold_ms * 1e3 / launches,
                       g_window_us_per_block=win_ms * 1e3 / win_blocks, g_eval_us_per_block=eval_ms * 1e3 / max(eval_launches, 1),
                       g_fold_kernel_s_per_1000=fold_ms * 1e-3 * 1000.0 / a.samples,
                       g_window_kernel_s_per_1000=win_ms * 1e-3 * 1000.0 / a.samples,
                       g_eval_kernel_s_per_1000=eval_ms * 1e-3 * 1000.0 / a.samples,
                       g_window_ks_D=r["ks_D"], g_window_min_log_sf=r["min_log_sf"], n_used=r["n_used"])
    return out


def scan_leg(a, w, y, P):
    """(i) the fold pass with the sliding-window scan off and on, and the kernels' own times."""
    widths = [int(t) for t in a.scan.split(",")]
    out = dict(i_scan_widths=widths, i_scan_like_p=a.like_p)
    with tamcmc_amd.Accel(2, w["plength"], w["x"], y, likelihood_p=float(a.like_p)) as acc:
        with tamcmc_amd.Summary(acc, a.block) as s0, tamcmc_amd.Summary(acc, a.block, scan=widths) as s1:
            times = {0: [], 1: []}
            for k in range(a.warmup + a.steps):
                for on, s in ((0, s0), (1, s1)):
                    s.reset()
                    acc.synchronize()
                    t0 = time.perf_counter()
                    s.push(P)                               # synchronous: results are on the host on return
                    if k >= a.warmup:
                        times[on].append(time.perf_counter() - t0)
            for on, key in ((0, "off"), (1, "on")):
                out[f"i_scan_{key}_s_per_1000"] = float(np.median(times[on])) * 1000.0 / a.samples
                out[f"i_scan_{key}_spread"] = [float(min(times[on])) * 1000.0 / a.samples, float(max(times[on])) * 1000.0 / a.samples]
            s1.reset()
            s1.profile(True)
            acc.profile(True)
            s1.push(P)
            fold_ms, launches = s1.kernel_time()
            scan_ms, scan_blocks = s1.scan_kernel_time()
            eval_ms, eval_launches = acc.kernel_time()
            acc.profile(False)
            s1.profile(False)
            res = [s1.scan_result(k) for k in range(len(widths))]
            out.update(i_scan_blocks=scan_blocks, i_scan_n_positions=[r["n_positions"] for r in res],
                       i_fold_us_per_block=fold_ms * 1e3 / launches, i_scan_us_per_block=scan_ms * 1e3 / scan_blocks,
                       i_eval_us_per_block=eval_ms * 1e3 / max(eval_launches, 1),
                       i_fold_kernel_s_per_1000=fold_ms * 1e-3 * 1000.0 / a.samples,
                       i_scan_kernel_s_per_1000=scan_ms * 1e-3 * 1000.0 / a.samples,
                       i_eval_kernel_s_per_1000=eval_ms * 1e-3 * 1000.0 / a.samples,
                       i_scan_min_log_sf=[r["min_log_sf"] for r in res], i_scan_pos_min_log_sf=[r["pos_min_log_sf"] for r in res],
                       i_scan_min_log_cdf=[r["min_log_cdf"] for r in res], i_scan_pos_min_log_cdf=[r["pos_min_log_cdf"] for r in res],
                       i_scan_regions_sf=[len(s1.scan_regions(k, 0)) for k in range(len(widths))],
                       i_scan_regions_cdf=[len(s1.scan_regions(k, 1)) for k in range(len(widths))], n_used=res[0]["n_used"])
    return out


def scan_null_leg(a):
    """(j) the Monte-Carlo null of the scan: wall time and kernel time per replicate."""
    widths = [int(t) for t in (a.scan or "10,20,40").split(",")]
    out = dict(j_scan_null_widths=widths, j_scan_null_like_p=a.like_p, j_scan_null_R_per_run=a.scan_null)
    with tamcmc_amd.ScanNull(0, a.like_p, a.nx, widths, 3) as null:
        times = []
        for k in range(a.warmup + a.steps):
            if k == a.warmup:
                null.profile(True)
            t0 = time.perf_counter()
            null.run(a.scan_null)                           # synchronous
            if k >= a.warmup:
                times.append(time.perf_counter() - t0)
        ms, chunks = null.kernel_time()
        null.profile(False)
        R = null.replicates
        out.update(j_scan_null_wall_s_per_replicate=float(np.median(times)) / a.scan_null,
                   j_scan_null_wall_spread=[float(min(times)) / a.scan_null, float(max(times)) / a.scan_null],
                   j_scan_null_kernel_s_per_replicate=ms * 1e-3 / (a.steps * a.scan_null), j_scan_null_chunks=chunks,
                   j_scan_null_additions_per_s=float(a.nx) * widths[-1] * a.steps * a.scan_null / (ms * 1e-3),
                   j_scan_null_replicates=R,
                   j_scan_null_joint_line=[null.line(k, 0, 0.01, True) for k in range(len(widths))] if R >= 99 else None,
                   j_scan_null_width_line=[null.line(k, 0, 0.01, False) for k in range(len(widths))] if R >= 99 else None,
                   j_scan_null_default_line=[float(np.log(0.01 * W / a.nx)) for W in widths])
    return out


def compare_leg(a):
    """(s) the comparison of fits: the bootstrap per replicate, the stacking per iteration, and one host thread."""
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    K, R = (int(t) for t in a.compare.split(","))
    N = a.nx
    rng = np.random.default_rng(20261021)
    elpd = rng.normal(-3.0, 1.0, N)[None, :] + 0.3 * rng.standard_t(5, (K, N)) + 0.02 * np.arange(K)[:, None]
    out = dict(s_compare_K=K, s_compare_R=R, s_compare_N=N)
    with tamcmc_amd.Compare(elpd, seed=12345) as cmp:
        cmp.bootstrap(min(R, 256))                          # warm-up: code objects, the chunk's buffers
        cmp.profile(True)
        t0 = time.perf_counter()
        cmp.bootstrap(R)                                    # synchronous
        wall = time.perf_counter() - t0
        ms, chunks = cmp.kernel_time(0)
        out.update(s_compare_bootstrap_wall_s_per_replicate=wall / R, s_compare_bootstrap_kernel_s_per_replicate=ms * 1e-3 / R,
                   s_compare_bootstrap_chunks=chunks, s_compare_variates_per_s=float(R) * cmp.n_included / (ms * 1e-3),
                   s_compare_prob=cmp.prob(1, 0)[0] / cmp.replicates, s_compare_weights_bma_plus=cmp.weights("pseudo_bma_plus").tolist())
        cmp.stacking(1e-8, 20)                              # warm-up
        for tag, scratch in (("table", 0), ("no_table", 1)):
            cmp.profile(True)
            t0 = time.perf_counter()
            st = cmp.stacking(1e-8, 2000, scratch_bytes=scratch)
            wall = time.perf_counter() - t0
            ms, launches = cmp.kernel_time(1)
            out.update({f"s_compare_stack_{tag}_iterations": st["iterations"], f"s_compare_stack_{tag}_converged": st["converged"],
                        f"s_compare_stack_{tag}_wall_s": wall, f"s_compare_stack_{tag}_kernel_s": ms * 1e-3,
                        f"s_compare_stack_{tag}_kernel_s_per_iteration": ms * 1e-3 / st["iterations"],
                        f"s_compare_stack_{tag}_launch_groups": launches})
        out.update(s_compare_stack_gap=st["gap"], s_compare_stack_w=st["w"].tolist())
        cmp.profile(False)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "compare_host_time")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(root, "tamcmc-c-_amd", "csrc"),
                        os.path.join(root, "tools", "compare_host_time.cpp"), "-o", exe], check=True)
        host = json.loads(subprocess.run([exe, str(N), str(K), str(4 if N > 1000000 else 16), "3"], check=True, capture_output=True, text=True).stdout)
    out.update(s_compare_host_bootstrap_s_per_replicate=host["host_bootstrap_ms_per_replicate"] * 1e-3,
               s_compare_host_stack_s_per_iteration=host["host_stack_ms_per_iteration"] * 1e-3,
               s_compare_host_over_bootstrap_kernel=host["host_bootstrap_ms_per_replicate"] * 1e-3 / out["s_compare_bootstrap_kernel_s_per_replicate"],
               s_compare_host_over_stack_kernel=host["host_stack_ms_per_iteration"] * 1e-3 / out["s_compare_stack_table_kernel_s_per_iteration"])
    return out


def ess_leg(a, w, y, P):
    """(h) the fold pass beside the ESS pass of the same rows, and the kernels' own times."""
    out = {}
    with tamcmc_amd.Accel(2, w["plength"], w["x"], y) as acc:
        with tamcmc_amd.Summary(acc, a.block) as s:
            times = {"fold": [], "ess": []}
            for k in range(a.warmup + a.steps):
                s.reset()
                acc.synchronize()
                t0 = time.perf_counter()
                s.push(P)                                   # synchronous: results are on the host on return
                t1 = time.perf_counter()
                L = s.ess_begin(a.ess)
                acc.synchronize()
                t2 = time.perf_counter()
                s.push(P)
                t3 = time.perf_counter()
                if k >= a.warmup:
                    times["fold"].append(t1 - t0)
                    times["ess"].append(t3 - t2)
                if k + 1 < a.warmup + a.steps:
                    s.ess_end()
            for key, v in times.items():
                out[f"h_ess_{key}_pass_s_per_1000"] = float(np.median(v)) * 1000.0 / a.samples
                out[f"h_ess_{key}_pass_spread"] = [float(min(v)) * 1000.0 / a.samples, float(max(v)) * 1000.0 / a.samples]
            acc.synchronize()
            t0 = time.perf_counter()
            r = s.ess_result()
            t_result = time.perf_counter() - t0
            s.profile(True)                                 # the finish kernel alone: a second result without another pass
            s.ess_result()
            fin_ms, fin_launches = s.kernel_time()
            s.profile(False)
            s.ess_end()
            s.reset()                                       # the kernels alone: a profiled fold pass, then a profiled ESS pass
            s.profile(True)
            acc.profile(True)
            s.push(P)
            fold_ms, fold_launches = s.kernel_time()
            eval_ms, eval_launches = acc.kernel_time()
            acc.profile(False)
            s.profile(False)
            s.ess_begin(a.ess)
            s.profile(True)
            s.push(P)
            ess_ms, ess_blocks = s.kernel_time()
            s.profile(False)
            s.ess_end()
            out.update(h_ess_lag=L, h_ess_blocks=ess_blocks, h_ess_us_per_block=ess_ms * 1e3 / ess_blocks,
                       h_ess_kernels_s_per_1000=ess_ms * 1e-3 * 1000.0 / a.samples,
                       h_fold_kernel_s_per_1000=fold_ms * 1e-3 * 1000.0 / a.samples,
                       h_eval_kernel_s_per_1000=eval_ms * 1e-3 * 1000.0 / a.samples,
                       h_ess_fma_per_s=2.0 * (L + 1) * a.nx * a.samples / (ess_ms * 1e-3),
                       h_ess_result_s=t_result, h_ess_finish_ms=fin_ms / max(fin_launches, 1),
                       h_ess_bytes=(32 * L + 1120) * a.nx + 32,
                       h_ess_min_ess_M=r["min_ess_M"], h_ess_min_ess_l=r["min_ess_l"], h_ess_max_rhat=r["max_rhat"],
                       h_ess_n_truncated_M=r["n_truncated_M"], n_used=r["n_used"])
    return out


def loo_pit_leg(a, w, y, P):
    """(l) the LOO tail pass beside the LOO-PIT pass of the same rows, and the kernels' own times."""
    out = dict(l_loo_pit_like_p=a.like_p)
    per_1000 = 1000.0 / a.samples
    with tamcmc_amd.Accel(2, w["plength"], w["x"], y, likelihood_p=float(a.like_p)) as acc:
        with tamcmc_amd.Summary(acc, a.block) as s:
            s.push(P)
            times = {"tail": [], "pit": [], "begin": []}
            for k in range(a.warmup + a.steps):             # every round in a mode of its own: begin, push, pit_begin, push, end
                s.loo_begin()
                acc.synchronize()
                t0 = time.perf_counter()
                s.push(P)                                   # synchronous: results are on the host on return
                t1 = time.perf_counter()
                s.loo_pit_begin()                           # ends in a device synchronise
                t2 = time.perf_counter()
                s.push(P)
                t3 = time.perf_counter()
                if k >= a.warmup:
                    times["tail"].append(t1 - t0)
                    times["begin"].append(t2 - t1)
                    times["pit"].append(t3 - t2)
                if k + 1 < a.warmup + a.steps:
                    s.loo_end()
            for key in ("tail", "pit"):
                v = times[key]
                out[f"l_loo_pit_{key}_pass_s_per_1000"] = float(np.median(v)) * per_1000
                out[f"l_loo_pit_{key}_pass_spread"] = [float(min(v)) * per_1000, float(max(v)) * per_1000]
            out["l_loo_pit_begin_s"] = float(np.median(times["begin"]))
            r = s.loo_pit_result()
            s.loo_end()
            s.loo_begin()                                   # the kernels alone: a profiled tail pass, prepare, a profiled PIT pass
            s.profile(True)
            acc.profile(True)
            s.push(P)
            tail_ms, tail_launches = s.kernel_time()
            eval_ms, eval_launches = acc.kernel_time()
            acc.profile(False)
            s.profile(True)                                 # (profile() starts the timers again)
            s.loo_pit_begin()
            prep_ms, _ = s.kernel_time()
            s.profile(True)
            s.push(P)
            pit_ms, pit_launches = s.loo_pit_kernel_time()
            s.profile(False)
            s.loo_end()
        with tamcmc_amd.Summary(acc, a.block, predictive=True) as s1:
            s1.push(P)
            s1.reset()
            s1.profile(True)
            s1.push(P)
            pred_ms, pred_launches = s1.predictive_kernel_time()
            s1.profile(False)
    n = r["n_used"]
    M = int(np.ceil(min(n / 5.0, 3.0 * np.sqrt(float(n)))))
    out.update(l_loo_pit_M=M, l_loo_pit_launches=pit_launches, l_loo_pit_us_per_block=pit_ms * 1e3 / pit_launches,
               l_loo_pit_kernel_s_per_1000=pit_ms * 1e-3 * per_1000, l_loo_pit_kernel_us_per_sample=pit_ms * 1e3 / a.samples,
               l_loo_tail_kernel_s_per_1000=tail_ms * 1e-3 * per_1000, l_loo_tail_kernel_us_per_sample=tail_ms * 1e3 / a.samples,
               l_predictive_kernel_s_per_1000=pred_ms * 1e-3 * per_1000, l_predictive_kernel_us_per_sample=pred_ms * 1e3 / a.samples,
               l_eval_kernel_s_per_1000=eval_ms * 1e-3 * per_1000, l_loo_pit_prepare_ms=prep_ms,
               l_loo_bytes=(M + 1) * a.nx * 8 + 52 * a.nx + 32, l_loo_pit_bytes=M * a.nx * 8 + 116 * a.nx + 36,
               l_loo_pit_ks_D=r["loo_ks_D"], l_loo_pit_min_log_sf=r["min_loo_log_sf"], l_loo_pit_min_is_ess=r["min_is_ess"], n_used=n)
    return out


def wloo_leg(a, w, y, P):
    """(m) the window-LOO pass and its PIT pass beside the per-bin LOO tail and LOO-PIT kernels of the same rows."""
    W = a.loo_window
    out = dict(m_wloo_W=W, m_wloo_like_p=a.like_p)
    per_1000 = 1000.0 / a.samples
    with tamcmc_amd.Accel(2, w["plength"], w["x"], y, likelihood_p=float(a.like_p)) as acc:
        with tamcmc_amd.Summary(acc, a.block) as s:
            s.push(P)
            times = {"tail": [], "pit": [], "begin": []}
            for k in range(a.warmup + a.steps):             # every round in a mode of its own: begin, push, pit_begin, push, end
                nw = s.wloo_begin(W)
                acc.synchronize()
                t0 = time.perf_counter()
                s.push(P)                                   # synchronous: results are on the host on return
                t1 = time.perf_counter()
                s.wloo_pit_begin()                          # ends in a device synchronise
                t2 = time.perf_counter()
                s.push(P)
                t3 = time.perf_counter()
                if k >= a.warmup:
                    times["tail"].append(t1 - t0)
                    times["begin"].append(t2 - t1)
                    times["pit"].append(t3 - t2)
                if k + 1 < a.warmup + a.steps:
                    s.wloo_end()
            for key in ("tail", "pit"):
                v = times[key]
                out[f"m_wloo_{key}_pass_s_per_1000"] = float(np.median(v)) * per_1000
                out[f"m_wloo_{key}_pass_spread"] = [float(min(v)) * per_1000, float(max(v)) * per_1000]
            out["m_wloo_pit_begin_s"] = float(np.median(times["begin"]))
            loo = s.wloo_result()
            r = s.wloo_pit_result()
            s.wloo_end()
            s.wloo_begin(W)                                 # the mode's kernels alone: a profiled pass, finalize, prepare, a profiled PIT pass
            s.profile(True)
            acc.profile(True)
            s.push(P)
            tail_ms, tail_launches = s.kernel_time()
            eval_ms, _ = acc.kernel_time()
            acc.profile(False)
            s.profile(True)                                 # (profile() starts the timers again)
            s.wloo_result()
            fin_ms, _ = s.kernel_time()
            s.profile(True)
            s.wloo_pit_begin()
            prep_ms, _ = s.kernel_time()
            s.profile(True)
            s.push(P)
            pit_ms, pit_launches = s.wloo_pit_kernel_time()
            s.profile(False)
            s.wloo_end()
            s.loo_begin()                                   # the per-bin kernels of the same rows, the same way
            s.profile(True)
            s.push(P)
            bin_tail_ms, _ = s.kernel_time()
            s.loo_pit_begin()
            s.profile(True)
            s.push(P)
            bin_pit_ms, _ = s.loo_pit_kernel_time()
            s.profile(False)
            s.loo_end()
    n = r["n_used"]
    M = int(np.ceil(min(n / 5.0, 3.0 * np.sqrt(float(n)))))
    B = -(-a.samples // tail_launches)                      # samples per block (the last block may be shorter)
    us = 1e3 / a.samples
    out.update(m_wloo_n_windows=nw, m_wloo_M=M, m_wloo_block_chains=B, m_wloo_launches=tail_launches,
               m_wloo_tail_kernels_us_per_sample=tail_ms * us, m_wloo_pit_kernels_us_per_sample=pit_ms * us,
               m_loo_tail_kernel_us_per_sample=bin_tail_ms * us, m_loo_pit_kernel_us_per_sample=bin_pit_ms * us,
               m_eval_kernel_us_per_sample=eval_ms * us, m_wloo_finalize_ms=fin_ms, m_wloo_prepare_ms=prep_ms,
               m_wloo_bytes=8 * (M + 1) * nw + 52 * nw + 32 + 8 * B * nw, m_wloo_pit_bytes=8 * M * nw + 116 * nw + 36 + 16 * B * nw,
               m_wloo_elpd_lwo=loo["elpd_lwo_total"], m_wloo_p_lwo=loo["p_lwo"], m_wloo_k_max=loo["k_max"], m_wloo_n_k_high=loo["n_k_high"],
               m_wloo_ks_D=r["loo_ks_D"], m_wloo_min_log_sf=r["min_loo_log_sf"], m_wloo_min_is_ess=r["min_is_ess"], n_used=n)
    return out


def modetable_leg(a, w, P):
    """(n) the mode table: push on the host clock, the derive and fold kernels alone, the quantile call."""
    out = {}
    q = [0.16, 0.5, 0.84, 0.025, 0.975, 0.0, 1.0, 0.25][:a.quantiles]
    with tamcmc_amd.Accel(2, w["plength"], w["x"], np.ones(a.nx)) as acc:
        with tamcmc_amd.ModeTable(acc, a.samples) as mt:
            push, kern, quant = [], [], []
            for k in range(a.warmup + a.steps):
                mt.reset()
                acc.synchronize()
                t0 = time.perf_counter()
                mt.push(P)                                  # synchronous
                t1 = time.perf_counter()
                ms, launches = mt.kernel_time()
                t2 = time.perf_counter()
                r = mt.quantiles(q)                         # synchronous
                t3 = time.perf_counter()
                if k >= a.warmup:
                    push.append(t1 - t0); kern.append(ms); quant.append(t3 - t2)
            res = mt.result()
            out.update(n_modetable_cols=mt.n_cols, n_modetable_mult=mt.n_mult, n_modetable_launches=launches,
                       n_modetable_push_s_per_1000=float(np.median(push)) * 1000.0 / a.samples,
                       n_modetable_push_spread=[float(min(push)) * 1000.0 / a.samples, float(max(push)) * 1000.0 / a.samples],
                       n_modetable_kernels_us_per_sample=float(np.median(kern)) * 1e3 / a.samples,
                       n_modetable_kernels_spread_us=[float(min(kern)) * 1e3 / a.samples, float(max(kern)) * 1e3 / a.samples],
                       n_modetable_Nq=len(q), n_modetable_quantiles_call_ms=float(np.median(quant)) * 1e3,
                       n_modetable_quantiles_spread_ms=[float(min(quant)) * 1e3, float(max(quant)) * 1e3],
                       n_modetable_table_bytes=8 * a.samples * mt.n_cols,
                       n_modetable_first_freq_quantiles=[float(v) for v in r["values"][:, 4]],
                       n_used=res["n_used"], n_rejected=res["n_rejected"])
    return out


def seismic_leg(a, w, P):
    """(q) the seismic indices: the same rows through a table without and a table with the indices enabled (reference row:
    params_true) -- push on the host clock, the derive and fold kernels (ModeTable.kernel_time), the indices kernel alone
    (ModeTable.seismic_kernel_time), and the quantile, ess and rank_diag calls of either table on the host clock."""
    out = {}
    q = [0.16, 0.5, 0.84]
    with tamcmc_amd.Accel(2, w["plength"], w["x"], np.ones(a.nx)) as acc:
        for tag in ("base", "indices"):
            with tamcmc_amd.ModeTable(acc, a.samples) as mt:
                if tag == "indices":
                    info = mt.enable_indices(w["params_true"])
                    out.update(q_seismic_index_cols=info["n_index_cols"], q_seismic_base_cols=info["n_base_cols"], q_seismic_n_radial=info["n_radial"],
                               q_seismic_dnu_ref=info["dnu_ref"], q_seismic_eps_ref=info["eps_ref"])
                push, kern, seis, quant, ess, rank = [], [], [], [], [], []
                for k in range(a.warmup + a.steps):
                    mt.reset()
                    acc.synchronize()
                    t0 = time.perf_counter()
                    mt.push(P)                                  # synchronous
                    t1 = time.perf_counter()
                    mt.quantiles(q)
                    t2 = time.perf_counter()
                    mt.ess(0)
                    t3 = time.perf_counter()
                    mt.rank_diag(0)
                    t4 = time.perf_counter()
                    if k >= a.warmup:
                        push.append(t1 - t0); kern.append(mt.kernel_time()[0]); seis.append(mt.seismic_kernel_time()[0])
                        quant.append(t2 - t1); ess.append(t3 - t2); rank.append(t4 - t3)
                res = mt.result()
                us = 1e3 / a.samples
                out.update({f"q_seismic_{tag}_cols": mt.n_cols, f"q_seismic_{tag}_block": min(4096, (1 << 23) // mt.n_cols),
                            f"q_seismic_{tag}_push_s_per_1000": float(np.median(push)) * 1000.0 / a.samples,
                            f"q_seismic_{tag}_derive_fold_us_per_sample": float(np.median(kern)) * us,
                            f"q_seismic_{tag}_derive_fold_spread_us": [float(min(kern)) * us, float(max(kern)) * us],
                            f"q_seismic_{tag}_quantiles_call_ms": float(np.median(quant)) * 1e3,
                            f"q_seismic_{tag}_ess_call_ms": float(np.median(ess)) * 1e3,
                            f"q_seismic_{tag}_rank_diag_call_ms": float(np.median(rank)) * 1e3,
                            f"q_seismic_{tag}_n_used": res["n_used"]})
                if tag == "indices":
                    out.update(q_seismic_kernel_us_per_sample=float(np.median(seis)) * us,
                               q_seismic_kernel_spread_us=[float(min(seis)) * us, float(max(seis)) * us],
                               q_seismic_kernel_launches=mt.seismic_kernel_time()[1])
    return out


def modediag_leg(a, w, P):
    """(o) the diagnostics of the mode table's columns: the kernels of an ess and of a cov call, the host's serial loops."""
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    with tamcmc_amd.Accel(2, w["plength"], w["x"], np.ones(a.nx)) as acc:
        with tamcmc_amd.ModeTable(acc, a.samples) as mt:
            mt.push(P)
            table_ms, table_launches = mt.kernel_time()
            n = mt.result()["n_used"]
            L = -1
            ess_k, ess_h, cov_k, cov_h = [], [], [], []
            for k in range(a.warmup + a.steps):
                if a.modes_ess >= 0:
                    ms0, _ = mt.diag_kernel_time()
                    t0 = time.perf_counter()
                    r = mt.ess(a.modes_ess)                  # synchronous
                    t1 = time.perf_counter()
                    L = r["lag"]
                    if k >= a.warmup:
                        ess_k.append(mt.diag_kernel_time()[0] - ms0); ess_h.append((t1 - t0) * 1e3)
                if a.modes_cov:
                    ms0, _ = mt.diag_kernel_time()
                    t0 = time.perf_counter()
                    mt.cov()                                # synchronous
                    t1 = time.perf_counter()
                    if k >= a.warmup:
                        cov_k.append(mt.diag_kernel_time()[0] - ms0); cov_h.append((t1 - t0) * 1e3)
            out.update(o_modediag_cols=mt.n_cols, o_modediag_n=n, o_modediag_table_kernels_ms=table_ms, o_modediag_table_launches=table_launches)
            if ess_k:
                out.update(o_modediag_lag=L, o_modediag_ess_kernels_ms=float(np.median(ess_k)), o_modediag_ess_kernels_spread_ms=[min(ess_k), max(ess_k)],
                           o_modediag_ess_call_ms=float(np.median(ess_h)), o_modediag_lag_fma=float(sum(n - k for k in range(L + 1))) * mt.n_cols,
                           o_modediag_min_ess=r["min_ess"], o_modediag_n_constant=r["n_constant"])
            if cov_k:
                out.update(o_modediag_cov_kernel_ms=float(np.median(cov_k)), o_modediag_cov_kernel_spread_ms=[min(cov_k), max(cov_k)],
                           o_modediag_cov_call_ms=float(np.median(cov_h)), o_modediag_cov_fma=float(n) * mt.n_cols * (mt.n_cols + 1) / 2)
            n_cols = mt.n_cols
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "modediag_host_time")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(root, "tamcmc-c-_amd", "csrc"),
                        os.path.join(root, "tools", "modediag_host_time.cpp"), "-o", exe], check=True)
        host = json.loads(subprocess.run([exe, str(n), str(n_cols), str(max(L, 0)), str(n_cols if a.modes_cov else 0)], check=True,
                                         capture_output=True, text=True).stdout)
    if ess_k:
        out.update(o_modediag_host_lag_ms=host["host_lag_ms"], o_modediag_host_over_ess_kernels=host["host_lag_ms"] / out["o_modediag_ess_kernels_ms"])
    if cov_k:
        out.update(o_modediag_host_cov_ms=host["host_cov_ms"], o_modediag_host_over_cov_kernel=host["host_cov_ms"] / out["o_modediag_cov_kernel_ms"])
    return out


def moderank_leg(a, w, P):
    """(p) the rank-normalised diagnostics of the mode table's columns: the kernels of a rank_diag call (sort, transform, mean,
    lag, finish together), the call, and the serial statements on one host thread (tools/moderank_host_time.cpp)."""
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    with tamcmc_amd.Accel(2, w["plength"], w["x"], np.ones(a.nx)) as acc:
        with tamcmc_amd.ModeTable(acc, a.samples) as mt:
            mt.push(P)
            table_ms, table_launches = mt.kernel_time()
            n = mt.result()["n_used"]
            ker, call = [], []
            for k in range(a.warmup + a.steps):
                ms0, l0 = mt.rank_kernel_time()
                t0 = time.perf_counter()
                r = mt.rank_diag(a.modes_rank)                # synchronous
                t1 = time.perf_counter()
                if k >= a.warmup:
                    ker.append(mt.rank_kernel_time()[0] - ms0); call.append((t1 - t0) * 1e3)
                launches = mt.rank_kernel_time()[1] - l0
            L, n_cols = r["lag"], mt.n_cols
            out.update(p_moderank_cols=n_cols, p_moderank_n=n, p_moderank_lag=L, p_moderank_table_kernels_ms=table_ms,
                       p_moderank_table_launches=table_launches, p_moderank_kernels_ms=float(np.median(ker)),
                       p_moderank_kernels_spread_ms=[min(ker), max(ker)], p_moderank_call_ms=float(np.median(call)),
                       p_moderank_call_spread_ms=[min(call), max(call)], p_moderank_launches=launches,
                       p_moderank_chunks=launches // 6, p_moderank_col_bytes=tamcmc_amd.capi.moderank_col_bytes(n, L),
                       p_moderank_min_ess_bulk=r["min_ess_bulk"], p_moderank_min_ess_tail=r["min_ess_tail"], p_moderank_max_rhat=r["max_rhat"],
                       p_moderank_n_constant=r["n_constant"])
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "moderank_host_time")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(root, "tamcmc-c-_amd", "csrc"),
                        os.path.join(root, "tools", "moderank_host_time.cpp"), "-o", exe], check=True)
        host = json.loads(subprocess.run([exe, str(n), str(n_cols), str(L)], check=True, capture_output=True, text=True).stdout)
    total = host["host_sort_ms"] + host["host_transform_ms"] + host["host_lag_ms"]
    out.update(p_moderank_host_sort_ms=host["host_sort_ms"], p_moderank_host_transform_ms=host["host_transform_ms"],
               p_moderank_host_lag_ms=host["host_lag_ms"], p_moderank_host_ms=total, p_moderank_host_over_kernels=total / out["p_moderank_kernels_ms"])
    return out


def modepdf_leg(a, w, P):
    """(r) histograms, shortest intervals and pair densities of the mode table's columns: per call the summed kernel time
    (ModeTable.pdf_kernel_time) and the wall time, the share of the sort launches in the hpd call, and the serial statements on
    one host thread (tools/modepdf_host_time.cpp)."""
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    with tamcmc_amd.Accel(2, w["plength"], w["x"], np.ones(a.nx)) as acc:
        with tamcmc_amd.ModeTable(acc, a.samples) as mt:
            mt.push(P)
            table_ms, table_launches = mt.kernel_time()
            n, n_cols = mt.result()["n_used"], mt.n_cols
            cols = mt.columns()
            K = tamcmc_amd.ModeTable.KINDS
            wcol = {int(c["mult"]): k for k, c in enumerate(cols) if K[c["kind"]] == "width"}
            hcol = {int(c["mult"]): k for k, c in enumerate(cols) if K[c["kind"]] == "height"}
            pairs = np.array([[wcol[m], hcol[m]] for m in sorted(wcol)], dtype=np.int32)
            edge = [k for k, c in enumerate(cols) if K[c["kind"]] in ("window_lo", "window_hi")]
            calls = (("hist", lambda: mt.hist(50)), ("hist_edges", lambda: mt.hist(50, edge)), ("hpd", lambda: mt.hpd([0.68, 0.95])),
                     ("hpd_sort", lambda: mt.hpd([1.0])),          # k = n: the window kernel has one start, the rest is the sort launch
                     ("hist2d", lambda: mt.hist2d(pairs, 32, mass=(0.68, 0.95))))
            for name, fn in calls:
                ker, call = [], []
                for k in range(a.warmup + a.steps):
                    ms0, l0 = mt.pdf_kernel_time()
                    t0 = time.perf_counter()
                    fn()                                         # synchronous
                    t1 = time.perf_counter()
                    if k >= a.warmup:
                        ker.append(mt.pdf_kernel_time()[0] - ms0); call.append((t1 - t0) * 1e3)
                    launches = mt.pdf_kernel_time()[1] - l0
                out.update({f"r_modepdf_{name}_kernels_ms": float(np.median(ker)), f"r_modepdf_{name}_kernels_spread_ms": [min(ker), max(ker)],
                            f"r_modepdf_{name}_call_ms": float(np.median(call)), f"r_modepdf_{name}_call_spread_ms": [min(call), max(call)],
                            f"r_modepdf_{name}_launches": launches})
            ms0 = mt.rank_kernel_time()[0]
            mt.rank_diag(1)
            out.update(r_modepdf_cols=n_cols, r_modepdf_n=n, r_modepdf_pairs=len(pairs), r_modepdf_edge_cols=len(edge),
                       r_modepdf_table_kernels_ms=table_ms, r_modepdf_table_launches=table_launches,
                       r_modepdf_rank_diag_kernels_ms=mt.rank_kernel_time()[0] - ms0)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "modepdf_host_time")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(root, "tamcmc-c-_amd", "csrc"),
                        os.path.join(root, "tools", "modepdf_host_time.cpp"), "-o", exe], check=True)
        host = json.loads(subprocess.run([exe, str(n), str(n_cols), str(len(pairs))], check=True, capture_output=True, text=True).stdout)
    out.update({"r_modepdf_" + k: v for k, v in host.items() if k != "host_sink"})
    return out


def bandess_leg(a, w, y, P):
    """(k) the fold pass beside the band ESS pass of the same rows, and the kernels' own times."""
    out = {}
    q = [0.025, 0.5, 0.975, 0.16, 0.84, 0.0, 1.0, 0.25][:a.quantiles]
    with tamcmc_amd.Accel(2, w["plength"], w["x"], y) as acc:
        with tamcmc_amd.Summary(acc, a.block) as s:
            s.push(P)
            thr = s.quantiles(P, q, a.qbits)["lo"]          # the exact quantiles: the thresholds of every pass below
            times = {"fold": [], "bandess": []}
            for k in range(a.warmup + a.steps):
                s.reset()
                acc.synchronize()
                t0 = time.perf_counter()
                s.push(P)                                   # synchronous: results are on the host on return
                t1 = time.perf_counter()
                L = s.bandess_begin(thr, a.band_ess)
                acc.synchronize()
                t2 = time.perf_counter()
                s.push(P)
                t3 = time.perf_counter()
                if k >= a.warmup:
                    times["fold"].append(t1 - t0)
                    times["bandess"].append(t3 - t2)
                if k + 1 < a.warmup + a.steps:
                    s.bandess_end()
            for key, v in times.items():
                out[f"k_bandess_{key}_pass_s_per_1000"] = float(np.median(v)) * 1000.0 / a.samples
                out[f"k_bandess_{key}_pass_spread"] = [float(min(v)) * 1000.0 / a.samples, float(max(v)) * 1000.0 / a.samples]
            acc.synchronize()
            t0 = time.perf_counter()
            r = s.bandess_result()
            t_result = time.perf_counter() - t0
            s.profile(True)                                 # the finish kernels alone: a second result without another pass
            s.bandess_result()
            fin_ms, fin_launches = s.kernel_time()
            s.profile(False)
            s.bandess_end()
            s.reset()                                       # the kernels alone: a profiled fold pass, then a profiled band pass
            s.profile(True)
            acc.profile(True)
            s.push(P)
            fold_ms, fold_launches = s.kernel_time()
            eval_ms, eval_launches = acc.kernel_time()
            acc.profile(False)
            s.profile(False)
            s.bandess_begin(thr, a.band_ess)
            s.profile(True)
            s.push(P)
            band_ms, band_blocks = s.kernel_time()
            s.profile(False)
            s.bandess_end()
            K = len(q)
            out.update(k_bandess_lag=L, k_bandess_K=K, k_bandess_blocks=band_blocks, k_bandess_us_per_block=band_ms * 1e3 / band_blocks,
                       k_bandess_kernels_s_per_1000=band_ms * 1e-3 * 1000.0 / a.samples,
                       k_fold_kernel_s_per_1000=fold_ms * 1e-3 * 1000.0 / a.samples,
                       k_eval_kernel_s_per_1000=eval_ms * 1e-3 * 1000.0 / a.samples,
                       k_bandess_counter_bytes_per_s=2.0 * 4 * K * (L + 1) * a.nx * band_blocks / (band_ms * 1e-3),
                       k_bandess_result_s=t_result, k_bandess_finish_ms_per_threshold=fin_ms / max(fin_launches, 1),
                       k_bandess_bytes=((4 * K + 8) * (L + 1) + 16 * K * (-(-L // 64) + 1) + 28 * K) * a.nx + 32,
                       k_bandess_min_ess=[float(v) for v in r["min_ess"]], k_bandess_n_truncated=[int(v) for v in r["n_truncated"]],
                       k_bandess_n_constant=[int(v) for v in r["n_constant"]], n_used=r["n_used"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--samples-b", type=int, default=256)
    ap.add_argument("--block", type=int, default=0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nx", type=int, default=100000)
    ap.add_argument("--quantiles", type=int, default=3)
    ap.add_argument("--qbits", type=int, default=0)
    ap.add_argument("--predictive", action="store_true")
    ap.add_argument("--like-p", type=int, default=1)
    ap.add_argument("--loo-pit", action="store_true", help="the LOO-PIT pass beside the LOO tail pass and the predictive kernel")
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--loo-window", type=int, default=0, help="W: the window-LOO pass and its PIT pass beside the per-bin LOO kernels")
    ap.add_argument("--scan", default="", help="W0[,W1,...]: strictly ascending widths of the sliding-window scan")
    ap.add_argument("--ess", type=int, default=-1)
    ap.add_argument("--band-ess", type=int, default=-1, help="L: the band ESS pass at --quantiles thresholds (0: the library's lag limit)")
    ap.add_argument("--modes", action="store_true", help="the posterior mode table: push, the derive and fold kernels, the quantile call")
    ap.add_argument("--modes-ess", type=int, default=-1, help="L: with --modes, ESS / MCSE / R-hat of the table's columns (0: the library's lag limit)")
    ap.add_argument("--modes-cov", action="store_true", help="with --modes, the covariance matrix of all columns")
    ap.add_argument("--modes-rank", type=int, default=-1, help="L: with --modes, the rank-normalised diagnostics of the table's columns (0: the library's lag limit)")
    ap.add_argument("--modes-indices", action="store_true", help="with --modes, the seismic indices: the indices kernel beside derive and fold, the "
                    "quantile, ess and rank_diag calls on the enlarged table beside the base table")
    ap.add_argument("--modes-pdf", action="store_true", help="with --modes, the histograms, shortest intervals and pair densities of the "
                    "table's columns beside derive and fold and beside one host thread")
    ap.add_argument("--scan-null", type=int, default=0, help="R: replicates per run of the scan's Monte-Carlo null (widths of --scan)")
    ap.add_argument("--compare", default="", help="K,R: the comparison of K fits over --nx units, R bootstrap replicates, and the stacking fit")
    a = ap.parse_args()
    if a.compare:
        out = dict(tool="summary_time", version=tamcmc_amd.capi.version())
        out.update(compare_leg(a))
        print(json.dumps(out))
        return
    if a.steps < 1 or a.warmup < 0 or a.samples < 1 or a.samples_b < 2 or a.scan_null < 0:
        ap.error("--steps >= 1, --warmup >= 0, --samples >= 1, --samples-b >= 2, --scan-null >= 0")
    if (a.modes_ess >= 0 or a.modes_cov or a.modes_rank >= 0 or a.modes_indices or a.modes_pdf) and not a.modes:
        ap.error("--modes-ess, --modes-cov, --modes-rank, --modes-indices and --modes-pdf need --modes")
    if a.scan_null:
        out = dict(tool="summary_time", Nx=a.nx, steps=a.steps, warmup=a.warmup, version=tamcmc_amd.capi.version())
        out.update(scan_null_leg(a))
        print(json.dumps(out))
        return
    w = synth.workload_c2(Nx=a.nx)
    P = synth.chain_params(w, a.samples)
    if a.modes:
        out = dict(tool="summary_time", Nx=a.nx, samples=a.samples, steps=a.steps, warmup=a.warmup, version=tamcmc_amd.capi.version())
        out.update(modepdf_leg(a, w, P) if a.modes_pdf else seismic_leg(a, w, P) if a.modes_indices else moderank_leg(a, w, P) if a.modes_rank >= 0 else modediag_leg(a, w, P) if a.modes_ess >= 0 or a.modes_cov else modetable_leg(a, w, P))
        print(json.dumps(out))
        return
    with tamcmc_amd.Accel(2, w["plength"], w["x"], np.ones(a.nx)) as acc:
        m_true, st = acc.model_explicit(w["params_true"])
    assert st == 0
    y = synth.make_spectrum(m_true)
    out = dict(tool="summary_time", Nx=a.nx, samples=a.samples, steps=a.steps, warmup=a.warmup, version=tamcmc_amd.capi.version())
    if a.loo_pit or a.loo_window:
        out.update(wloo_leg(a, w, y, P) if a.loo_window else loo_pit_leg(a, w, y, P))
        print(json.dumps(out))
        return
    if a.predictive or a.window or a.scan or a.ess >= 0 or a.band_ess >= 0:
        out.update(bandess_leg(a, w, y, P) if a.band_ess >= 0 else ess_leg(a, w, y, P) if a.ess >= 0 else scan_leg(a, w, y, P) if a.scan else window_leg(a, w, y, P) if a.window
                   else predictive_leg(a, w, y, P))
        print(json.dumps(out))
        return
    with tamcmc_amd.Accel(2, w["plength"], w["x"], y) as acc:
        with tamcmc_amd.Summary(acc, a.block) as s:
            for _ in range(a.warmup):
                s.push(P)
            times = []
            for _ in range(a.steps):
                s.reset()
                acc.synchronize()
                t0 = time.perf_counter()
                s.push(P)                                   # synchronous: results are on the host on return
                times.append(time.perf_counter() - t0)
            res = s.result()
            out["a_summary_s_per_1000"] = float(np.median(times)) * 1000.0 / a.samples
            out["a_spread"] = [float(min(times)) * 1000.0 / a.samples, float(max(times)) * 1000.0 / a.samples]
            out["n_used"], out["n_rejected"] = res["n_used"], res["n_rejected"]
            # (c) the fold kernel alone
            s.reset()
            s.profile(True)
            s.push(P)
            ms, launches = s.kernel_time()
            s.profile(False)
            B = -(-a.samples // launches)                   # samples per block (the last block may be shorter)
            bytes_moved = (a.samples * a.nx + launches * 2 * 8 * a.nx) * 8.0
            out.update(c_fold_launches=launches, c_block_chains=B, c_fold_us_per_block=ms * 1e3 / launches,
                       c_fold_s_per_1000=ms * 1e-3 * 1000.0 / a.samples, c_fold_bytes_per_s=bytes_moved / (ms * 1e-3),
                       c_fold_share_of_copy_ceiling=bytes_moved / (ms * 1e-3) / COPY_CEILING)
            # (d) quantile mode: the same rows again, once per pass, until every value is exact
            s.reset()
            s.push(P)
            q = [0.16, 0.5, 0.84, 0.025, 0.975, 0.0, 1.0, 0.25][:a.quantiles]
            s.quantiles_begin(q, a.qbits)
            pass_times, left = [], None
            while left != 0:
                acc.synchronize()
                t0 = time.perf_counter()
                s.push(P)
                left = s.quantiles_step()                   # synchronises the stream
                pass_times.append(time.perf_counter() - t0)
            s.quantiles_end()
            s.quantiles_begin(q, a.qbits)                   # the histogram kernel alone, over the first pass
            s.profile(True)
            s.push(P)
            ms, launches = s.kernel_time()
            s.profile(False)
            s.quantiles_end()
            out.update(d_quantile_Nq=len(q), d_quantile_bits=a.qbits or 6, d_quantile_passes=len(pass_times),
                       d_quantile_s_per_pass_per_1000=float(np.median(pass_times)) * 1000.0 / a.samples,
                       d_quantile_spread=[float(min(pass_times)) * 1000.0 / a.samples, float(max(pass_times)) * 1000.0 / a.samples],
                       d_quantile_total_s_per_1000=float(np.sum(pass_times)) * 1000.0 / a.samples,
                       d_quantile_hist_us_per_block=ms * 1e3 / launches, d_quantile_hist_s_per_1000=ms * 1e-3 * 1000.0 / a.samples,
                       d_quantile_hist_bytes=len(q) * (1 << (a.qbits or 6)) * a.nx * 4)
            # (e) LOO mode: the same rows once more, then the finalize kernel
            s.reset()
            s.push(P)
            tail_times = []
            for k in range(a.warmup + a.steps):             # every pass in a mode of its own: begin, push, (result,) end
                s.loo_begin()
                acc.synchronize()
                t0 = time.perf_counter()
                s.push(P)
                if k >= a.warmup:
                    tail_times.append(time.perf_counter() - t0)
                if k + 1 < a.warmup + a.steps:
                    s.loo_end()
            acc.synchronize()
            t0 = time.perf_counter()
            loo = s.loo_result()
            t_result = time.perf_counter() - t0
            s.profile(True)                                 # the finalize kernel alone: a second result without another pass
            s.loo_result()
            fin_ms, fin_launches = s.kernel_time()
            s.profile(False)
            s.loo_end()
            s.loo_begin()                                   # the tail kernel alone, over one pass
            s.profile(True)
            s.push(P)
            ms, launches = s.kernel_time()
            s.profile(False)
            s.loo_end()
            M = int(np.ceil(min(res["n_used"] / 5.0, 3.0 * np.sqrt(float(res["n_used"])))))
            out.update(e_loo_M=M, e_loo_tail_s_per_1000=float(np.median(tail_times)) * 1000.0 / a.samples,
                       e_loo_tail_spread=[float(min(tail_times)) * 1000.0 / a.samples, float(max(tail_times)) * 1000.0 / a.samples],
                       e_loo_tail_us_per_block=ms * 1e3 / launches, e_loo_tail_kernel_s_per_1000=ms * 1e-3 * 1000.0 / a.samples,
                       e_loo_result_s=t_result, e_loo_finalize_ms=fin_ms / max(fin_launches, 1),
                       e_loo_bytes=(M + 1) * a.nx * 8 + 52 * a.nx + 32,
                       e_loo_k_max=loo["k_max"], e_loo_n_k_high=loo["n_k_high"], e_loo_n_k_inf=loo["n_k_inf"],
                       e_loo_elpd=loo["elpd_loo_total"], e_loo_p_loo=loo["p_loo"], e_p_waic=res["p_waic"])
        # (b) the host route, on fewer rows
        Pb = P[:a.samples_b]
        host_fold(acc, Pb[:64], y)
        t0 = time.perf_counter()
        ref = host_fold(acc, Pb, y)
        out["b_host_route_s_per_1000"] = (time.perf_counter() - t0) * 1000.0 / len(Pb)
        out["b_samples"] = len(Pb)
        # same numbers from both routes (the recurrences are the same; numpy's log / exp differ from the device's in the last bits)
        with tamcmc_amd.Summary(acc, a.block) as s:
            s.push(Pb)
            r2 = s.result()
        out["ab_max_rel_diff"] = {k: float(np.max(np.abs(r2[k] - ref[k]) / np.maximum(np.abs(ref[k]), 1e-300)))
                                  for k in ("mean_M", "var_M", "lppd", "var_l")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
