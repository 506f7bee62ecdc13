"""Parameter rows for every model id of models_ctrl.list: derived from the synthetic C2 star (tamcmc_amd.synth) by
make / any_model, and of any lmax, Harvey background and grid by layout.  Test helper only."""
import math

import numpy as np

import tamcmc_amd
from tamcmc_amd import synth


def _base(Nx, lmax=2, asym=0.0, trunc_c=20.0, do_amp=False):
    w = synth.workload_c2(model_case=2, Nx=Nx, asym=asym, trunc_c=trunc_c, do_amp=do_amp)
    return w


def split(w):
    """Blocks of a global params row."""
    pl = w["plength"]
    Nmax, lmax = int(pl[0]), int(pl[1])
    Nf = int(pl[2] + pl[3] + pl[4] + pl[5])
    s = Nmax + lmax + Nf
    wq = s + int(pl[6])
    z = wq + int(pl[7])
    q = z + int(pl[8])
    return dict(Nmax=Nmax, lmax=lmax, Nf=Nf, s=s, w=wq, z=z, q=q, cfg=q + int(pl[9]))


def make(model_case, Nx=4096, asym=0.0, trunc_c=20.0, do_amp=False, seed=7):
    """Returns (plength, params, index_to_relax) for `model_case` on the C2 grid (first Nx bins... the grid
    is rescaled so that all 21 modes stay inside it)."""
    rng = np.random.default_rng(seed)
    w = _base(100000, asym=asym, trunc_c=trunc_c, do_amp=do_amp)
    x = synth.grid(Nx, 2300.0, 840.0 / Nx)
    p = w["params_true"].copy()
    pl = w["plength"].copy()
    b = split(w)
    Nmax, lmax, s, wq, z, q, cfg = b["Nmax"], b["lmax"], b["s"], b["w"], b["z"], b["q"], b["cfg"]
    relax = w["relax"].copy()
    if do_amp:
        p[:Nmax] = p[:Nmax] * math.pi * p[wq:wq + Nmax]   # amplitudes^2 giving similar heights
    if model_case in (2,):
        pass
    elif model_case == 3:
        w3 = synth.workload_c2(model_case=3, Nx=100000, asym=asym, trunc_c=trunc_c, do_amp=do_amp)
        relax = w3["relax"].copy()
    elif model_case in (6, 7, 8):
        extra = {6: 1, 7: Nmax, 8: 2 * Nmax}[model_case]
        a1 = 1.4
        head, tail = p[:s + 6], p[s + 6:]
        ext = a1 * (1.0 + 0.2 * rng.standard_normal(extra))
        if model_case == 6:
            ext = np.array([0.9])         # a1(l=2) < 1 while a1(l=1) > 1: both window branches
        p = np.concatenate([head, ext, tail])
        p[s] = a1
        pl[6] = 6 + extra
        relax = np.concatenate([relax[:s + 6], np.ones(extra, dtype=np.int32), relax[s + 6:]])
        relax[s] = 1
        relax[s + 3] = relax[s + 4] = 0
        relax[-3] = 1     # inclination
    elif model_case in (9, 10):
        if model_case == 9:
            wp = [2600.0, 4.0, 2.0, 3500.0, 2.0]
        else:
            wp = [2700.0, 2600.0, 4.0, 2.0, 3500.0, 2.0]
        p = np.concatenate([p[:wq], wp, p[wq + Nmax:]])
        relax = np.concatenate([relax[:wq], np.ones(len(wp), dtype=np.int32), relax[wq + Nmax:]])
        pl[7] = len(wp)
    elif model_case == 12:
        r = [0.33, 0.335, 0.0001, 0.33, 0.17, 0.05, 0.15, 0.28, 0.09]
        p = np.concatenate([p[:q], r, p[q + 1:]])
        relax = np.concatenate([relax[:q], np.ones(9, dtype=np.int32), relax[q + 1:]])
        pl[9] = 9
        p[s] = 1.4; relax[s] = 1; relax[s + 3] = relax[s + 4] = 0
    elif model_case == 13:
        nh = (lmax + 1) * (Nmax - 1) + lmax + 1
        h = 0.2 + rng.random(nh)
        if do_amp:
            h = h * 3.0
        p = np.concatenate([p[:q], h, p[q + 1:]])
        relax = np.concatenate([relax[:q], np.ones(nh, dtype=np.int32), relax[q + 1:]])
        pl[9] = nh
        p[s] = 1.4; relax[s] = 1; relax[s + 3] = relax[s + 4] = 0
        relax[Nmax:Nmax + lmax] = 0       # visibilities are not used by this model
    else:
        raise ValueError(model_case)
    return dict(model_case=model_case, plength=pl.astype(np.int32), params_true=p, x=x,
                index_to_relax=np.flatnonzero(relax).astype(np.int32), relax=relax)


def make_local(model_case, Nx=4096, asym=0.0, trunc_c=20.0, do_amp=False, seed=11):
    rng = np.random.default_rng(seed)
    w = synth.workload_c1(Nx=10000, trunc_c=trunc_c)
    x = synth.grid(Nx, 94.30, 81.2 / Nx)
    p = w["params_true"].copy()
    pl = w["plength"].copy()
    relax = w["relax"].copy()
    Nf = [int(v) for v in pl[2:6]]
    Nmax = int(pl[0])
    s = Nmax + int(pl[1]) + sum(Nf)
    p[s + 5] = asym
    cfg = len(p) - 2
    p[cfg + 1] = 1.0 if do_amp else 0.0
    if do_amp:
        wq = s + int(pl[6])
        p[:Nmax] = p[:Nmax] * math.pi * p[wq:wq + Nmax]
    if model_case == 11:
        pass
    elif model_case == 14:
        # heights block: l=0 -> Nfl0 entries, then the reference's literal (overlapping) indexing
        # off_l + (l+1) n + |m|; make the block long enough for every read
        need = 0
        off = 0
        for l in range(4):
            if Nf[l] > 0:
                need = max(need, off + (l + 1) * (Nf[l] - 1) + l + 1)
            off += Nf[l]
        NmaxH = max(need, Nmax)
        h = 0.5 + 10.0 * rng.random(NmaxH)
        p = np.concatenate([h, p[Nmax:]])
        relax = np.concatenate([np.ones(NmaxH, dtype=np.int32), relax[Nmax:]])
        pl[0] = NmaxH
        s = NmaxH + int(pl[1]) + sum(Nf)
        p[s] = 0.4; relax[s] = 1; relax[s + 3] = relax[s + 4] = 0
    else:
        raise ValueError(model_case)
    return dict(model_case=model_case, plength=pl.astype(np.int32), params_true=p, x=x,
                index_to_relax=np.flatnonzero(relax).astype(np.int32), relax=relax)


def make_gauss(model_case, Nx=4096):
    x = synth.grid(Nx, 1000.0, 2000.0 / Nx)
    if model_case == 0:
        p = np.array([5.0, 150.0, 2100.0, 0.7])
        pl = [4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    else:
        p = np.array([5.0, -150.0, 2100.0, 3.0, 2.5, 2.2, 0.7])
        pl = [3, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0]
    return dict(model_case=model_case, plength=np.array(pl, dtype=np.int32), params_true=p, x=x,
                index_to_relax=np.arange(p.size, dtype=np.int32), relax=np.ones(p.size, dtype=np.int32))


def any_model(model_case, **kw):
    if model_case in (0, 1):
        kw.pop("asym", None); kw.pop("trunc_c", None); kw.pop("do_amp", None)
        return make_gauss(model_case, **kw)
    if model_case in (11, 14):
        return make_local(model_case, **kw)
    return make(model_case, **kw)


def perturbed(w, Nchains, scale=0.01, seed=3):
    """Chains = truth * (1 + scale * N(0,1)) on the relaxed entries."""
    rng = np.random.default_rng(seed)
    P = np.tile(w["params_true"], (Nchains, 1))
    idx = w["index_to_relax"]
    P[:, idx] *= 1.0 + scale * rng.standard_normal((Nchains, idx.size))
    return P


ALL_IDS = [0, 1, 2, 3, 6, 7, 8, 9, 10, 11, 12, 13, 14]
LAYOUT_IDS = (2, 3, 6, 7, 8, 9, 10, 12, 13)     # global ids: layout() at any lmax


# ---------------------------------------------------------------------------------------------------------------------
# Layouts beyond the C2 star: every global id at lmax = 0..3, local ids with l = 3 modes, 0..3 Harvey profiles.

NOISE_C2 = ((0.0, 0.0, 1.0), (11.049588, 49.669854, 4.0), (0.93569041, 1.3516447, 2.0))   # synth._KPLR_NOISE[:9]
WHITE_C2 = 0.13392108


def _layout_modes(Nmax, lmax, n0=38, Dnu=60.0, eps=1.4, D0=0.9):
    """(nu, Gamma, H) per degree, asymptotic pattern of synth.workload_c4; widths 0.7 ... 2.5 so that the window takes
    both its Gamma < 1 and Gamma > 1 branches."""
    numax = Dnu * (n0 + Nmax / 2.0 + eps)
    modes = []
    for l in range(lmax + 1):
        row = []
        for k in range(Nmax):
            nu = Dnu * (n0 + k + l / 2.0 + eps) - l * (l + 1) * D0
            G = 0.7 + 1.8 * k / max(Nmax - 1, 1)
            H = 2.0 * math.exp(-0.5 * ((nu - numax) / (3.0 * Dnu)) ** 2)
            row.append((nu, G, H))
        modes.append(row)
    return modes


def _noise_block(noise, white):
    """noise: 0..3 (H, tau, p) tuples -> the 10 entries of the reference's noise block; unused slots tau = 0."""
    noise = [tuple(float(v) for v in h) for h in noise]
    assert len(noise) <= 3
    blk = []
    for h in noise + [(0.0, 0.0, 0.0)] * (3 - len(noise)):
        blk.extend(h)
    return blk + [float(white)]


def _noise_relax(relax, z, blk):
    """H and tau of every active profile (tau != 0) are variables, and so is p where it is not 0 (at p = 0 the profile
    is the constant H/2 and |p| has no derivative); the white noise always."""
    for k in range(3):
        act = blk[3 * k + 1] != 0.0
        relax[z + 3 * k] = relax[z + 3 * k + 1] = int(act)
        relax[z + 3 * k + 2] = int(act and blk[3 * k + 2] != 0.0)
    relax[z + 9] = 1


def layout(mid, lmax=2, noise=NOISE_C2, white=WHITE_C2, asym=0.0, trunc_c=20.0, do_amp=False, Nmax=5, Nx=3000,
           grid=None, shape_vars=None, seed=7):
    """Returns a workload dict (plength, params_true, relax, index_to_relax, x, model_case) of global id `mid` with
    degrees 0..lmax and Nmax radial orders, or of a local id (11, 14) with one or two modes of every degree 0..3
    (lmax is then ignored).

    The id-specific blocks follow models.cpp / io_ms_global.cpp of the reference:
      6  Nsplit = 7: a1(l=1) at s, a1(l=2) at s+6;             7  Nsplit = 6 + Nmax: a1 per n at s+6+n;
      8  Nsplit = 6 + 2 Nmax: a1 per n for l=1, then for l=2;  9 / 10  Nwidth = 5 / 6 (Appourchaux widths);
      12 Ninc = 2 + 3 [lmax>=2] + 4 [lmax>=3] m-height ratios; 13 Ninc = (lmax+1)(Nmax-1) + lmax + 1 heights.
    noise: 0..3 Harvey profiles (H, tau, p); any sign, p = 0 and tau = 0 (profile off) allowed.
    grid: (x0, step) of the Nx bins; default: the modes' range plus margins.
    shape_vars: eta, a3 and the asymmetry are variables (default: where asym != 0; with the asymmetry a variable the
    gradient launch takes the asymmetric code path even at asym = 0)."""
    if shape_vars is None:
        shape_vars = asym != 0.0
    if mid in (11, 14):
        return _local_layout(mid, noise_white=white, asym=asym, trunc_c=trunc_c, do_amp=do_amp, Nx=Nx, grid=grid,
                             shape_vars=shape_vars, seed=seed)
    assert mid in (2, 3, 6, 7, 8, 9, 10, 12, 13) and 0 <= lmax <= 3 and Nmax >= 2
    rng = np.random.default_rng(seed)
    modes = _layout_modes(Nmax, lmax)
    if grid is None:
        lo = min(m[0] for row in modes for m in row) - 25.0
        hi = max(m[0] for row in modes for m in row) + 25.0
        grid = (lo, (hi - lo) / Nx)
    x = synth.grid(Nx, grid[0], grid[1])
    blk = _noise_block(noise, white)
    w = synth._global_workload(3 if mid == 3 else 2, modes, [1.5, 0.53, 0.2], 1.4, 55.0, 1e-5, 0.01, asym, blk,
                               trunc_c, do_amp, x)
    p, pl, relax = w["params_true"].copy(), w["plength"].copy(), w["relax"].copy()
    s, wq = Nmax + lmax + Nmax * (lmax + 1), Nmax + lmax + Nmax * (lmax + 1) + 6
    z = wq + Nmax
    q = z + 10
    _noise_relax(relax, z, blk)
    if do_amp:
        p[:Nmax] = p[:Nmax] * math.pi * p[wq:wq + Nmax]   # amplitudes^2 giving similar heights
    if mid in (6, 7, 8, 12, 13):
        # a1 (or the a1 blocks) given directly: the sqrt(a1) cos i / sin i pair is unused
        relax[s] = int(mid in (6, 12, 13))
        relax[s + 3] = relax[s + 4] = 0
    if mid in (6, 7, 8):
        relax[q] = 1      # the inclination
        extra = {6: 1, 7: Nmax, 8: 2 * Nmax}[mid]
        ext = np.array([0.9]) if mid == 6 else 1.4 * (1.0 + 0.2 * rng.standard_normal(extra))
        if mid == 8:
            ext[Nmax:] = np.abs(ext[Nmax:] - 0.6)       # a1(l=2) < 1 where a1(l=1) > 1: both window branches
        p = np.concatenate([p[:s + 6], ext, p[s + 6:]])
        relax = np.concatenate([relax[:s + 6], np.ones(extra, dtype=np.int32), relax[s + 6:]])
        pl[6] = 6 + extra
    elif mid in (9, 10):
        f0 = np.array([m[0] for m in modes[0]])
        c = float(np.mean(f0))
        wp = [c - 60.0, 4.0, 1.2, 1.3 * c, 2.0] if mid == 9 else [c, c - 60.0, 4.0, 1.2, 1.3 * c, 2.0]
        p = np.concatenate([p[:wq], wp, p[wq + Nmax:]])
        relax = np.concatenate([relax[:wq], np.ones(len(wp), dtype=np.int32), relax[wq + Nmax:]])
        pl[7] = len(wp)
    elif mid == 12:
        nr = 2 + (3 if lmax >= 2 else 0) + (4 if lmax >= 3 else 0)
        r = [0.33, 0.335, 0.0001, 0.33, 0.17, 0.05, 0.15, 0.28, 0.09][:nr]
        p = np.concatenate([p[:q], r, p[q + 1:]])
        relax = np.concatenate([relax[:q], np.full(nr, int(lmax >= 1), dtype=np.int32), relax[q + 1:]])
        pl[9] = nr
    elif mid == 13:
        nh = (lmax + 1) * (Nmax - 1) + lmax + 1
        h = 0.2 + rng.random(nh)
        if do_amp:
            h = h * 3.0
        p = np.concatenate([p[:q], h, p[q + 1:]])
        relax = np.concatenate([relax[:q], np.full(nh, int(lmax >= 1), dtype=np.int32), relax[q + 1:]])
        pl[9] = nh
        relax[Nmax:Nmax + lmax] = 0       # visibilities are not used by this model
    if shape_vars:
        relax[[s + 1, s + 2, s + 5]] = 1
    assert p.size == int(pl.sum()) == relax.size
    return dict(model_case=mid, plength=pl.astype(np.int32), params_true=p, x=x,
                index_to_relax=np.flatnonzero(relax).astype(np.int32), relax=relax)


# (l, nu, Gamma, H) of the local layouts: synth.workload_c1's modes plus two l = 3 modes
_LOCAL_MODES = [(0, 110.2, 0.15, 12.0), (0, 152.8, 0.18, 9.0), (1, 131.5, 0.16, 14.0), (1, 168.9, 0.2, 7.0),
                (2, 105.6, 0.17, 6.0), (2, 148.1, 0.19, 5.0), (3, 124.9, 0.17, 4.0), (3, 161.3, 1.3, 3.0)]


def _local_layout(mid, noise_white=0.8, asym=0.0, trunc_c=20.0, do_amp=False, Nx=3000, grid=None, shape_vars=False,
                  seed=11):
    """model_MS_local_basic (11) / model_MS_local_Hnlm (14) rows with modes of degrees 0..3 (synth.workload_c1's layout:
    heights, frequencies, 6 splitting entries, widths, N0, inclination, trunc_c, do_amp)."""
    rng = np.random.default_rng(seed)
    by_l = [[m for m in _LOCAL_MODES if m[0] == l] for l in range(4)]
    Nf = [len(b) for b in by_l]
    Nmodes = sum(Nf)
    a1, inc = 0.4, math.radians(60.0)
    H = [m[3] for b in by_l for m in b]
    F = [m[1] for b in by_l for m in b]
    G = [m[2] for b in by_l for m in b]
    split = [a1, 0.0, 0.0, math.sqrt(a1) * math.cos(inc), math.sqrt(a1) * math.sin(inc), asym]
    rsplit = [0, 0, 0, 1, 1, 0]
    if mid == 14:
        split[0] = 0.4
        rsplit = [1, 0, 0, 0, 0, 0]
    if shape_vars:
        rsplit[1] = rsplit[2] = rsplit[5] = 1
    if grid is None:
        grid = (94.30, 81.2 / Nx)
    x = synth.grid(Nx, grid[0], grid[1])
    if mid == 11:
        heights = np.array(H)
        if do_amp:
            heights = heights * math.pi * np.array(G)
    else:
        # heights block: l=0 -> Nfl0 entries, then the reference's literal (overlapping) indexing off_l + (l+1) n + |m|
        need, off = 0, 0
        for l in range(4):
            if Nf[l] > 0:
                need = max(need, off + (l + 1) * (Nf[l] - 1) + l + 1)
            off += Nf[l]
        heights = 0.5 + 10.0 * rng.random(max(need, Nmodes))
        if do_amp:
            heights = heights * 0.6
    Nh = heights.size
    p = np.concatenate([heights, F, split, G, [noise_white, 60.0, trunc_c, 1.0 if do_amp else 0.0]])
    relax = np.concatenate([np.ones(Nh + Nmodes, dtype=np.int32), rsplit, np.ones(Nmodes, dtype=np.int32), [1, 0, 0, 0]])
    pl = np.array([Nh, 0] + Nf + [6, Nmodes, 1, 1, 2], dtype=np.int32)
    assert p.size == int(pl.sum()) == relax.size
    return dict(model_case=mid, plength=pl, params_true=p, x=x, index_to_relax=np.flatnonzero(relax).astype(np.int32),
                relax=relax.astype(np.int32))


def local_asymptotic(Nfl=(4, 3, 4, 2), dnu=14.0, eps=1.3, d0=0.15, n0=6, asym=0.0, do_amp=False):
    """id 11 with Nfl modes per degree on the asymptotic pattern nu = dnu (n + l / 2 + eps) - l (l + 1) d0: a local layout with
    enough radial modes for the seismic indices (_local_layout's params row: heights, frequencies, 6 splitting entries, widths,
    N0, inclination, trunc_c, do_amp)."""
    Nx = 3000
    F = [dnu * (n0 + k + l / 2.0 + eps) - l * (l + 1) * d0 for l in range(4) for k in range(Nfl[l])]
    nm = len(F)
    H = [12.0 - 0.5 * j for j in range(nm)]
    G = [0.15 + 0.005 * j for j in range(nm)]
    if do_amp:
        H = [h * math.pi * g for h, g in zip(H, G)]
    a1, inc = 0.4, math.radians(60.0)
    split = [a1, 0.0, 0.0, math.sqrt(a1) * math.cos(inc), math.sqrt(a1) * math.sin(inc), asym]
    p = np.array(H + F + split + G + [0.8, 60.0, 20.0, 1.0 if do_amp else 0.0])
    relax = np.concatenate([np.ones(2 * nm, dtype=np.int32), [0, 0, 0, 1, 1, 0], np.ones(nm, dtype=np.int32), [1, 0, 0, 0]]).astype(np.int32)
    pl = np.array([nm, 0] + list(Nfl) + [6, nm, 1, 1, 2], dtype=np.int32)
    assert p.size == int(pl.sum()) == relax.size
    return dict(model_case=11, plength=pl, params_true=p, x=synth.grid(Nx, 94.30, 81.2 / Nx), index_to_relax=np.flatnonzero(relax).astype(np.int32),
                relax=relax)


def poly_cells(w, params=None):
    """Number of cells (8 * 512 bins) of one chain whose Harvey background the device evaluates as a Taylor polynomial,
    and the number of cells.  Mirrors the rule of tamcmc_setup_body.h (every active profile h: |p_h| * span <= 0.04 and
    t0 = (1e-3 |tau_h| x_c)^|p_h| < 1e290, span = the cell's half-width in log x) -- a PRECONDITION check for tests that
    want both kinds of cells in one chain, not a statement of what the device does."""
    p = w["params_true"] if params is None else params
    pl = w["plength"]
    x = w["x"]
    if w["model_case"] in (11, 14):
        profiles = []
    else:
        z = int(pl[:8].sum())
        nh = (int(pl[8]) - 1) // 3
        profiles = [(abs(p[z + 3 * k + 1]), abs(p[z + 3 * k + 2])) for k in range(nh)]
        profiles = [(t, e) for (t, e) in profiles if t != 0 and e != 0]
    lx = np.log(x)
    Nx, cb = x.size, 8 * 512
    cells = (Nx + cb - 1) // cb
    npoly = 0
    for ce in range(cells):
        base = ce * cb
        TB = min(cb, Nx - base)
        ic, i1 = min(base + TB // 2, Nx - 1), min(base + TB - 1, Nx - 1)
        span = max(abs(lx[base] - lx[ic]), abs(lx[i1] - lx[ic]))
        ok = True
        for (tau, e) in profiles:
            ok = ok and e * span <= 0.04 and math.exp(e * (math.log(1e-3 * tau) + lx[ic])) < 1e290
        npoly += int(ok)
    return npoly, cells
