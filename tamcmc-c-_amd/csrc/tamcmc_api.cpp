// tamcmc_api.cpp -- host side of the C ABI declared in include/tamcmc_accel.h.
// Owns the device buffers of one context, validates arguments the way Model_def's callers rely on
// (plength sums to Nparams, model / likelihood ids from the *.list tables), and strings the launches of
// one evaluation on the context stream:
//     setup (params -> multiplet table, tile descriptors)
//     -> eval (model + likelihood; the last workgroup of a chain sums its tiles in fixed order: -p(..)/T)
//     or eval<grad> (+ gradient partials) -> backward (tile sums, chain rule to d/dvars, logL)
// No CPU fallback exists in this library.  Fit groups are in tamcmc_group.cpp, posterior summaries in
// tamcmc_summary_api.cpp; what the three share is in tamcmc_host.h.
#include <cmath>
#include <cstdlib>
#include <new>
#include <type_traits>

#include "tamcmc_host.h"

thread_local char tm_hip_err[256] = "";

// What most entry points ask of their context first: it is there, and no armed batch waits behind its gate (only _fire /
// _end / _disarm / destroy are accepted meanwhile, tamcmc_accel.h).
static bool ctx_usable(const tamcmc_ctx *c) { return c && !c->armed; }
static uint32_t *gate_word(const tamcmc_ctx *c) { return c->gate.host<uint32_t>(); }   // (NULL before the first _arm)

static int model_supported(int id)
{
    if (id == 4 || id == 5) return TAMCMC_E_MODEL_DISABLED;
    if (id < 0 || id > 14) return TAMCMC_E_UNKNOWN_MODEL;
    return TAMCMC_OK;
}

// Build the layout of the params row (models.cpp:492-506, :1696-1710).
static int build_layout(TmLayout &L, int model_case, int likelihood_case, double like_p, const int32_t plength[11],
                        int64_t Nx, const double *x)
{
    std::memset(&L, 0, sizeof(L));
    L.model_case = model_case;
    L.likelihood_case = likelihood_case;
    L.like_p = (double)(long)like_p;           // `long p`, likelihoods.cpp:17
    L.Nx = (int32_t)Nx;
    L.x0 = x[0];
    L.xlast = x[Nx - 1];
    L.step = x[1] - x[0];
    int sum = 0;
    for (int i = 0; i < 11; i++) { if (plength[i] < 0) return TAMCMC_E_INVALID; sum += plength[i]; }
    L.Nparams = sum;
    if (model_case == 0 || model_case == 1) {
        L.family = TM_FAM_GAUSS;
        L.n_mult = 0;
        if (sum < (model_case == 0 ? 4 : 7)) return TAMCMC_E_INVALID;
        L.nharvey = (model_case == 1) ? 1 : 0;
        return TAMCMC_OK;
    }
    L.family = (model_case == 11 || model_case == 14) ? TM_FAM_LOCAL : TM_FAM_GLOBAL;
    L.variant = (model_case == 6 || model_case == 7 || model_case == 8) ? 1 : ((model_case == 13 || model_case == 14) ? 2 : 0);
    L.Nmax = plength[0];
    L.lmax = plength[1];
    for (int l = 0; l < 4; l++) L.Nfl[l] = plength[2 + l];
    L.Nsplit = plength[6]; L.Nwidth = plength[7]; L.Nnoise = plength[8]; L.Ninc = plength[9];
    const int Nf = L.Nfl[0] + L.Nfl[1] + L.Nfl[2] + L.Nfl[3];
    L.off_f[0] = L.Nmax + L.lmax;
    for (int l = 1; l < 4; l++) L.off_f[l] = L.off_f[l - 1] + L.Nfl[l - 1];
    L.s = L.Nmax + L.lmax + Nf;
    L.w = L.s + L.Nsplit;
    L.z = L.w + L.Nwidth;
    L.q = L.z + L.Nnoise;
    if (L.q + L.Ninc + 2 > sum) return TAMCMC_E_INVALID;   // trunc_c and do_amp must exist
    if (L.Nsplit < 6) return TAMCMC_E_INVALID;
    if (L.Nnoise < 1) return TAMCMC_E_INVALID;
    if (L.family == TM_FAM_GLOBAL) {
        if (L.lmax < 0 || L.lmax > 3 || L.Nmax < 1) return TAMCMC_E_INVALID;
        for (int l = 0; l <= L.lmax; l++) if (L.Nfl[l] != L.Nmax) return TAMCMC_E_INVALID; // models.cpp:485-486
        L.n_mult = L.Nmax * (L.lmax + 1);
        if (L.n_mult > TM_MAXMULT) return TAMCMC_E_INVALID;
        L.nharvey = (L.Nnoise - 1) / 3;
        if (L.nharvey > TM_MAXH) return TAMCMC_E_INVALID;
        const bool interp = !(model_case == 9 || model_case == 10);
        if (interp && L.lmax >= 1 && L.Nfl[0] < 2) return TAMCMC_E_INVALID;  // lin_interpol needs two nodes
        if (interp && L.Nwidth < L.Nmax) return TAMCMC_E_INVALID;
        if (model_case == 9 && L.Nwidth < 5) return TAMCMC_E_INVALID;
        if (model_case == 10 && L.Nwidth < 6) return TAMCMC_E_INVALID;
        if (model_case == 6 && L.Nsplit < 7) return TAMCMC_E_INVALID;
        if (model_case == 7 && L.Nsplit < 6 + L.Nmax) return TAMCMC_E_INVALID;
        if (model_case == 8 && L.Nsplit < 6 + 2 * L.Nmax) return TAMCMC_E_INVALID;
        if (model_case == 12 && L.Ninc < 2 + (L.lmax >= 2 ? 3 : 0) + (L.lmax >= 3 ? 4 : 0)) return TAMCMC_E_INVALID;
        if (model_case == 13 && L.lmax >= 1 && L.Ninc < (L.lmax + 1) * (L.Nmax - 1) + L.lmax + 1) return TAMCMC_E_INVALID;
        if ((model_case == 3 || model_case == 6 || model_case == 7 || model_case == 8) && L.Ninc < 1) return TAMCMC_E_INVALID;
    } else {
        L.n_mult = Nf;
        if (L.n_mult > TM_MAXMULT) return TAMCMC_E_INVALID;
        L.nharvey = 0;                         // models.cpp:1818
        if (Nf < 1) return TAMCMC_E_INVALID;
        if (L.Nwidth < Nf) return TAMCMC_E_INVALID;
        if (model_case == 11 && L.Nmax < Nf) return TAMCMC_E_INVALID;
        if (model_case == 14) {
            int off = 0;
            for (int l = 0; l < 4; l++) {
                if (L.Nfl[l] > 0 && off + (l + 1) * (L.Nfl[l] - 1) + l >= sum) return TAMCMC_E_INVALID;
                off += L.Nfl[l];
            }
        }
    }
    return TAMCMC_OK;
}

// The per-batch buffers live in ONE allocation (a slab, carved at 256-byte boundaries): the kernels of a step touch a
// dozen of them within their first microseconds, and every separate hipMalloc sits in pages of its own.
static void free_batch(tamcmc_ctx *c)
{
    (void)hipFree(c->d_slab); c->d_slab = nullptr;
    c->d_params = c->d_T = c->d_logL = c->d_part = c->d_gmult = c->d_gnoise = c->d_hser = c->d_wt = nullptr;
    c->d_status = c->d_rows = c->d_order = c->d_ticket = nullptr;
    c->d_mult = nullptr; c->d_noise = nullptr; c->d_cell = nullptr; c->d_thdr = nullptr; c->d_tidx = nullptr;
    c->d_chain_rec = c->d_aux = nullptr;
    c->cap = 0; c->cap_grad = false;
}

int tm_ensure_capacity(tamcmc_ctx *c, int Nchains, bool grad)
{
    if (!tm_batch_fits(c, Nchains, grad)) return TAMCMC_E_INVALID;   // before anything is sized for a batch no launch can take
    if (Nchains <= c->cap && (!grad || c->cap_grad)) return TAMCMC_OK;
    const int cap = Nchains > c->cap ? Nchains : c->cap;
    const bool g = grad || c->cap_grad;
    TM_HIP(tm_ctx_stream_sync(c));
    free_batch(c);
    const size_t n = (size_t)cap;
    const size_t nm = (size_t)(c->L.n_mult > 0 ? c->L.n_mult : 1);
    // two passes over the same list: sizes first, then the pointers
    char *base = nullptr;
    size_t off = 0;
    auto carve = [&](auto **ptr, size_t bytes) {
        if (base) *ptr = reinterpret_cast<std::remove_reference_t<decltype(**ptr)> *>(base + off);
        off += (bytes + 255) & ~(size_t)255;
    };
    auto layout = [&]() {
        off = 0;
        carve(&c->d_params, n * c->L.Nparams * sizeof(double));
        carve(&c->d_T, n * sizeof(double));
        carve(&c->d_logL, n * sizeof(double));
        carve(&c->d_wt, n * 2 * sizeof(double));
        carve(&c->d_status, n * sizeof(int32_t));
        carve(&c->d_rows, n * sizeof(int32_t));
        carve(&c->d_ticket, n * sizeof(int32_t));
        carve(&c->d_noise, n * sizeof(TmNoise));
        carve(&c->d_order, n * c->tiles_max * sizeof(int32_t));
        carve(&c->d_thdr, n * c->tiles_max * sizeof(TmTileHdr));
        carve(&c->d_part, n * c->tiles_max * 4 * sizeof(double));
        carve(&c->d_cell, n * c->cells * sizeof(TmCellRec));
        carve(&c->d_mult, n * nm * sizeof(TmMult));
        carve(&c->d_tidx, n * c->tiles_max * nm * sizeof(TmActive));
        if (g) {
            char *cr = nullptr, *ax = nullptr;
            carve(&cr, n * tm_sizeof_chain_rec());
            carve(&ax, n * nm * tm_sizeof_aux());
            if (base) { c->d_chain_rec = cr; c->d_aux = ax; }
            carve(&c->d_gnoise, n * c->tiles_g * 2 * TM_NSLOTS * sizeof(double));
            carve(&c->d_hser, n * c->cells * TM_MAXH * TM_HSER * sizeof(double));
            carve(&c->d_gmult, n * c->tiles_g * nm * TM_GSLOTS * sizeof(double));
        }
    };
    layout();
    const size_t total = off;
    if (hipMalloc(&c->d_slab, total) != hipSuccess) { c->d_slab = nullptr; free_batch(c); return TAMCMC_E_NOMEM; }
    base = static_cast<char *>(c->d_slab);
    layout();
    TM_HIP(hipMemset(c->d_ticket, 0, n * sizeof(int32_t)));
    c->cap = cap;
    c->cap_grad = g;
    return TAMCMC_OK;
}

extern "C" int tamcmc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int tamcmc_ctx_create(tamcmc_ctx **out, int device_id, int model_case, int likelihood_case,
                                 double likelihood_p, const int32_t plength[11], int64_t Nx,
                                 const double *x, const double *y, const double *sigma_y)
{
    if (!out) return TAMCMC_E_INVALID;
    *out = nullptr;
    if (!plength || !x || !y || Nx < 2 || Nx > (1LL << 28)) return TAMCMC_E_INVALID;   // 32-bit byte offsets in the eval kernel (the reference reads at most 1e6 rows, config.cpp:531)
    int rc = model_supported(model_case);
    if (rc != TAMCMC_OK) return rc;
    if (likelihood_case != 0 && likelihood_case != 1) return TAMCMC_E_UNKNOWN_MODEL;
    if (likelihood_case == 1 && !sigma_y) return TAMCMC_E_INVALID;
    const int ndev = tamcmc_device_count();
    if (ndev <= 0 || device_id < 0 || device_id >= ndev) return TAMCMC_E_NODEVICE;

    tamcmc_ctx *c = new (std::nothrow) tamcmc_ctx();
    if (!c) return TAMCMC_E_NOMEM;
    c->device = device_id;
    rc = build_layout(c->L, model_case, likelihood_case, likelihood_p, plength, Nx, x);
    if (rc != TAMCMC_OK) { delete c; return rc; }

    auto env_int = [](const char *name, int lo, int hi, int *dst) {
        const char *e = getenv(name);
        if (e) { int v = atoi(e); if (v >= lo && v <= hi) *dst = v; }
    };
    // Developer switches (documented in include/tamcmc_accel.h); none of them changes a result beyond rounding.
    { int v = 0; env_int("TAMCMC_BG_EXACT", 0, 1, &v); c->L.bg_exact = v; }
    env_int("TAMCMC_ORDER", 0, 2, &c->order_mode);
    env_int("TAMCMC_FUSED", 0, 1, &c->fuse);
    env_int("TAMCMC_EQUAL_COST", 0, 1, &c->equal_cost);
    env_int("TAMCMC_GATE_PATIENCE", 1, 1 << 30, &c->gate_patience);
    env_int("TAMCMC_PRIO", 0, 1, &c->prio);
    auto env_cost = [](const char *name, TmCostModel *m) {
        const char *e = getenv(name);
        int c0, a, b;
        // accepted only while the balancer's int32 cost prefix cannot overflow: the worst unit costs
        // c0 + TM_MAXMULT * (7 a + b) and at most TM_EQ_MAXU units are balanced (tm_tile_bound itself works in 64 bit);
        // a model outside that range is ignored (the defaults stay) rather than clamped
        if (e && sscanf(e, "%d,%d,%d", &c0, &a, &b) == 3 && c0 >= 1 && c0 <= 10000 && a >= 0 && a <= 1000 && b >= 0 && b <= 1000 &&
            ((long long)c0 + (long long)TM_MAXMULT * (7LL * a + b)) * (long long)TM_EQ_MAXU < (1LL << 31)) { m->c0 = c0; m->a = a; m->b = b; }
    };
    env_cost("TAMCMC_COST", &c->cost_l);
    env_cost("TAMCMC_COST_GRAD", &c->cost_g);
    {
        c->units = tm_units(Nx);
        c->cells = tm_cells(c->units);
        c->tiles_l = tm_tiles(c->units, 0);
        c->tiles_g = tm_tiles(c->units, 1);
        // a tile count given by hand must still keep every tile within TM_TILE_MAXU units
        const int tmin_g = (c->units + TM_TILE_MAXU - 1) / TM_TILE_MAXU + (c->units > TM_TILE_MAXU ? 1 : 0);
        const int tmin_l = (c->units + TM_TILE_MAXU_L - 1) / TM_TILE_MAXU_L + (c->units > TM_TILE_MAXU_L ? 1 : 0);
        if (c->units > 4) {
            env_int("TAMCMC_TILES", tmin_l, 1 << 20, &c->tiles_l);
            env_int("TAMCMC_TILES_GRAD", tmin_g, 1 << 20, &c->tiles_g);
        }
        // Tail shaping of the gradient launch (long grids, equal-length tiles): the first tiles keep TM_TILE_MAXU units, the
        // rest -- cheaper, hence launched last under the costliest-first order -- get su2 units, so that the workgroups
        // that end the launch are short (the launch is 1.56 rounds of resident workgroups at C2, and a round's last
        // workgroups run on a nearly empty chip).  The long tiles cover `frac` percent of the units: 85 %, 4 units by
        // default -- at 1e5 bins 21 tiles of 8 units + 7 of 4 (measured, profiles/README.md: C2 80.2 -> 78.1 us, C4 258 ->
        // 251 us, 16 / 32 chains -1.1 us, 256 chains +1 %).  TAMCMC_TAIL="frac,su2" sets it, TAMCMC_TAIL=0 switches it off.
        // A function of the grid only, like the tile count: a chain's result does not depend on the batch.
        c->cost_g.t1 = 0;
        {
            const char *e = getenv("TAMCMC_TAIL");
            int frac = 85, su2 = 4;
            if (e && sscanf(e, "%d,%d", &frac, &su2) != 2) frac = 0;
            if (frac >= 1 && frac <= 99 && su2 >= 1 && su2 <= TM_TILE_MAXU &&
                c->units >= 70 && !c->equal_cost && !getenv("TAMCMC_TILES_GRAD")) {
                const int t1 = (int)(((long long)c->units * frac / 100 + TM_TILE_MAXU / 2) / TM_TILE_MAXU);
                const int rest = c->units - t1 * TM_TILE_MAXU;
                if (t1 >= 1 && rest > 0) {
                    c->cost_g.t1 = t1; c->cost_g.su1 = TM_TILE_MAXU; c->cost_g.su2 = su2;
                    c->tiles_g = t1 + (rest + su2 - 1) / su2;
                }
            }
        }
        // the balancer's guarantee is TM_TILE_MAXU units per tile; equal-length likelihood tiles may be longer
        c->cost_l.pad = (c->equal_cost && (long long)c->tiles_l * TM_TILE_MAXU > c->units) ? TM_TILE_MAXU : TM_TILE_MAXU_L;
    }
    c->tiles_max = c->tiles_l > c->tiles_g ? c->tiles_l : c->tiles_g;

    auto fail = [&](int code) { tamcmc_ctx_destroy(c); return code; };
    if (hipSetDevice(device_id) != hipSuccess) return fail(TAMCMC_E_NODEVICE);
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) return fail(TAMCMC_E_HIP);
    c->stream = c->own_stream;
    const size_t bytes = (size_t)Nx * sizeof(double);
    if (hipMalloc(&c->d_x2, bytes) != hipSuccess || hipMalloc(&c->d_y, bytes) != hipSuccess ||
        hipMalloc(&c->d_lx, bytes) != hipSuccess)
        return fail(TAMCMC_E_NOMEM);
    std::vector<double> tmp((size_t)Nx);
    for (int64_t i = 0; i < Nx; i++) tmp[(size_t)i] = 2.0 * x[i];        // exact; the Lorentzians are written in d = 2x - 2nu
    if (hipMemcpy(c->d_x2, tmp.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(TAMCMC_E_HIP);
    // log x table for the Harvey powers.  x == 0 (the first bin of a spectrum made by an FFT) is stored as -1e300, not -inf:
    // t = exp(p (lt - 1e300)) is exactly 0 while p * 1e300 exceeds about 745, i.e. for every Harvey exponent p >= 1e-297,
    // so u = 1 and the model are as with -inf, while the gradient's t u^2 (lt + log x) is 0 * finite = 0, the limit of
    // t ln(sx), and not 0 * inf = NaN.  The cell's span |p (log x - lxc)| is about p * 1e300 there, far above the 0.04 a
    // polynomial cell needs, so the cell that holds x == 0 takes the exp path.  An exponent below 1e-297 (p == 0 among
    // them) together with x == 0 is not supported: t is no longer 0, the cell may pass for a polynomial one and the weight
    // moments then overflow (include/tamcmc_accel.h).
    for (int64_t i = 0; i < Nx; i++) tmp[(size_t)i] = x[i] == 0.0 ? -1e300 : std::log(x[i]);
    if (hipMemcpy(c->d_y, y, bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->d_lx, tmp.data(), bytes, hipMemcpyHostToDevice) != hipSuccess)
        return fail(TAMCMC_E_HIP);
    if (likelihood_case == 1) {
        for (int64_t i = 0; i < Nx; i++) tmp[(size_t)i] = 1.0 / (sigma_y[i] * sigma_y[i]);  // likelihoods.cpp:36
        if (hipMalloc(&c->d_isig2, bytes) != hipSuccess) return fail(TAMCMC_E_NOMEM);
        if (hipMemcpy(c->d_isig2, tmp.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(TAMCMC_E_HIP);
    }
    *out = c;
    return TAMCMC_OK;
}

extern "C" int tamcmc_ctx_destroy(tamcmc_ctx *c)
{
    if (!c) return TAMCMC_OK;
    if (c->groups > 0) return TAMCMC_E_INVALID;     // a fit group still refers to it: destroy the group first
    if (c->summaries > 0) return TAMCMC_E_INVALID;  // and so does a summary object
    if (c->modetables > 0) return TAMCMC_E_INVALID; // or a mode table
    (void)hipSetDevice(c->device);
    if (c->armed && gate_word(c)) { __atomic_store_n(gate_word(c), c->gate_seq, __ATOMIC_RELEASE); c->armed = 0; }   // let the gate go
    if (c->stream) (void)tm_ctx_stream_sync(c);
    free_batch(c);
    c->gate.release();
    (void)hipFree(c->d_x2); (void)hipFree(c->d_y); (void)hipFree(c->d_lx); (void)hipFree(c->d_isig2); (void)hipFree(c->d_spec);
    (void)hipFree(c->d_model); (void)hipFree(c->d_relax);
    c->h_in.release(); c->h_out.release(); c->h_status.release();
    if (c->probe_stream) { (void)hipStreamSynchronize(c->probe_stream); (void)hipStreamDestroy(c->probe_stream); }
    c->probe.release();
    if (c->ev_done) (void)hipEventDestroy(c->ev_done);
    c->timer.destroy();
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return TAMCMC_OK;
}

extern "C" int tamcmc_ctx_set_vars(tamcmc_ctx *c, int32_t Nvars, const int32_t *index_to_relax)
{
    if (!ctx_usable(c) || c->in_flight || Nvars < 0 || (Nvars > 0 && !index_to_relax)) return TAMCMC_E_INVALID;
    // Every index in range and none twice (so Nvars <= Nparams): the backward kernel routes a pair to its variable through
    // the inverse of this list, and a parameter listed twice would have two columns of which an undefined one gets the
    // gradient and the other 0.  The reference's list comes from flags and cannot repeat (model_def.cpp:81-88).  Checked
    // before anything is freed or waited for: a refusal leaves the context as it was.
    {
        std::vector<char> seen((size_t)c->L.Nparams, 0);
        for (int i = 0; i < Nvars; i++) {
            const int32_t r = index_to_relax[i];
            if (r < 0 || r >= c->L.Nparams || seen[(size_t)r]) return TAMCMC_E_INVALID;
            seen[(size_t)r] = 1;
        }
    }
    // a layout whose gradient tables outgrow the backward kernel's LDS (every entry a variable: from some 210 to 235 multiplets on)
    // is refused here, the context left as it was -- not at the first gradient batch, after two of its three launches
    if (Nvars > 0 && !tm_backward_fits(c->L, c->tiles_g, Nvars)) return TAMCMC_E_NOGRAD;
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(tm_ctx_stream_sync(c));
    (void)hipFree(c->d_relax); c->d_relax = nullptr;
    c->Nvars = Nvars;
    // the asymmetry as a variable: its derivative does not vanish at asym == 0 although the factor is 1 there
    c->L.asym_var = 0;
    if (c->L.family != TM_FAM_GAUSS)
        for (int i = 0; i < Nvars; i++)
            if (index_to_relax[i] == c->L.s + 5) c->L.asym_var = 1;
    if (Nvars > 0) {
        TM_HIP(hipMalloc(&c->d_relax, (size_t)Nvars * sizeof(int32_t)));
        TM_HIP(hipMemcpy(c->d_relax, index_to_relax, (size_t)Nvars * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_ctx_set_spectra(tamcmc_ctx *c, int32_t Nspectra, const double *y, const double *sigma_y)
{
    if (!ctx_usable(c) || Nspectra < 1 || !y || (c->L.likelihood_case == 1 && !sigma_y)) return TAMCMC_E_INVALID;
    if (c->summaries > 0) return TAMCMC_E_INVALID;  // a summary's running state belongs to the resident spectrum
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(tm_ctx_stream_sync(c));
    const size_t nx = (size_t)c->L.Nx, bytes = nx * (size_t)Nspectra * sizeof(double);
    // the new blocks first, the swap last: a failure leaves the context as it was
    double *ny = nullptr, *nis = nullptr;
    if (hipMalloc(&ny, bytes) != hipSuccess) return TAMCMC_E_NOMEM;
    if (hipMemcpy(ny, y, bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(ny); return TAMCMC_E_HIP; }
    if (c->L.likelihood_case == 1) {
        std::vector<double> tmp(nx * (size_t)Nspectra);
        for (size_t i = 0; i < tmp.size(); i++) tmp[i] = 1.0 / (sigma_y[i] * sigma_y[i]);  // likelihoods.cpp:36
        if (hipMalloc(&nis, bytes) != hipSuccess) { (void)hipFree(ny); return TAMCMC_E_NOMEM; }
        if (hipMemcpy(nis, tmp.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(ny); (void)hipFree(nis); return TAMCMC_E_HIP; }
    }
    (void)hipFree(c->d_y); c->d_y = ny;
    if (c->L.likelihood_case == 1) { (void)hipFree(c->d_isig2); c->d_isig2 = nis; }
    (void)hipFree(c->d_spec); c->d_spec = nullptr; c->spec_n = 0;
    c->nspec = Nspectra;
    return TAMCMC_OK;
}

extern "C" int tamcmc_ctx_set_chain_spectrum(tamcmc_ctx *c, int32_t Nchains, const int32_t *spectrum_of_chain)
{
    if (!ctx_usable(c) || Nchains < 0 || (Nchains > 0 && !spectrum_of_chain)) return TAMCMC_E_INVALID;
    for (int m = 0; m < Nchains; m++)
        if (spectrum_of_chain[m] < 0 || spectrum_of_chain[m] >= c->nspec) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(tm_ctx_stream_sync(c));
    (void)hipFree(c->d_spec); c->d_spec = nullptr; c->spec_n = 0;
    if (Nchains > 0) {
        TM_HIP(hipMalloc(&c->d_spec, (size_t)Nchains * sizeof(int32_t)));
        TM_HIP(hipMemcpy(c->d_spec, spectrum_of_chain, (size_t)Nchains * sizeof(int32_t), hipMemcpyHostToDevice));
        c->spec_n = Nchains;
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_ctx_set_stream(tamcmc_ctx *c, void *hip_stream)
{
    if (!ctx_usable(c)) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(tm_ctx_stream_sync(c));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    c->enq_seq++;
    return TAMCMC_OK;
}

extern "C" int tamcmc_ctx_synchronize(tamcmc_ctx *c)
{
    if (!ctx_usable(c)) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(tm_ctx_stream_sync(c));
    return TAMCMC_OK;
}

extern "C" int tamcmc_ctx_profile(tamcmc_ctx *c, int enable)
{
    if (!c) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(tm_ctx_stream_sync(c));
    c->profile = enable != 0;
    c->profile_stride = enable > 1 ? enable : 1;
    c->profile_count = 0;
    c->timer.used = 0;
    // a pool of events up front: creating one costs ~10 us, which would land inside the caller's timed region
    return c->profile ? c->timer.pool(256) : TAMCMC_OK;
}

extern "C" int tamcmc_ctx_kernel_time(tamcmc_ctx *c, double *total_ms, int64_t *launches)
{
    if (!ctx_usable(c) || !total_ms || !launches) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(tm_ctx_stream_sync(c));
    return c->timer.total(total_ms, launches);
}

// One wave that does nothing but watch two counters for `ticks` ticks of the constant 100 MHz clock: s_memtime counts
// shader-core cycles, s_memrealtime the constant clock, so their ratio is the core clock the GPU ran at meanwhile --
// launched on a stream of its own beside the evaluation, it reads the clock UNDER THAT LOAD (bench.py: roofline.valu).
__global__ void tamcmc_clock_probe_kernel(unsigned long long ticks, unsigned long long *out)
{
    if (threadIdx.x != 0) return;
    const unsigned long long r0 = wall_clock64(), c0 = clock64();
    unsigned long long r1 = r0, c1 = c0;
    while (r1 - r0 < ticks) { __builtin_amdgcn_s_sleep(32); r1 = wall_clock64(); c1 = clock64(); }
    out[0] = c1 - c0;
    out[1] = r1 - r0;
}

extern "C" int tamcmc_ctx_clock_probe_begin(tamcmc_ctx *c, double milliseconds)
{
    if (!c || !(milliseconds > 0.0) || milliseconds > 2000.0) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(c->device));
    if (!c->probe_stream) TM_HIP(hipStreamCreateWithFlags(&c->probe_stream, hipStreamNonBlocking));
    const int rc = c->probe.reserve(2 * sizeof(unsigned long long), TM_PIN_MAPPED);
    if (rc != TAMCMC_OK) return rc;
    std::memset(c->probe.h, 0, 2 * sizeof(unsigned long long));
    hipLaunchKernelGGL(tamcmc_clock_probe_kernel, dim3(1), dim3(64), 0, c->probe_stream,
                       (unsigned long long)(milliseconds * 1e5), c->probe.dev<unsigned long long>());
    TM_HIP(hipGetLastError());
    return TAMCMC_OK;
}

extern "C" int tamcmc_ctx_clock_probe_end(tamcmc_ctx *c, double *core_GHz, double *seconds)
{
    if (!c || !c->probe_stream || !core_GHz) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(hipStreamSynchronize(c->probe_stream));
    const unsigned long long *const h_probe = c->probe.host<unsigned long long>();
    const double cyc = (double)h_probe[0], t = (double)h_probe[1] / 1e8;
    *core_GHz = (t > 0.0) ? cyc / t / 1e9 : 0.0;
    if (seconds) *seconds = t;
    return TAMCMC_OK;
}

extern "C" int tamcmc_ctx_geometry(tamcmc_ctx *c, int32_t *bins_per_tile, int32_t *tiles, int32_t *threads_per_block,
                                   int32_t *n_multiplets)
{
    if (!c) return TAMCMC_E_INVALID;
    const int T = c->last_tiles > 0 ? c->last_tiles : tm_ctx_tiles(c, false);
    if (bins_per_tile) *bins_per_tile = TM_UNIT_BINS * c->cost_l.pad;   // largest tile of the likelihood launch (TM_TILE_MAXU_L units; TM_TILE_MAXU when balanced, and always for the gradient launch)
    if (tiles) *tiles = T;
    if (threads_per_block) *threads_per_block = TM_THREADS;
    if (n_multiplets) *n_multiplets = c->L.n_mult;
    return TAMCMC_OK;
}

extern "C" int tamcmc_ctx_geometry_grad(tamcmc_ctx *c, int32_t *tiles, int32_t *bins_per_tile)
{
    if (!c) return TAMCMC_E_INVALID;
    if (tiles) *tiles = tm_ctx_tiles(c, true);
    if (bins_per_tile) *bins_per_tile = TM_UNIT_BINS * TM_TILE_MAXU;
    return TAMCMC_OK;
}

// Arguments of the eval launch of a batch on the context (solo launches and fit groups alike).
TmEvalArgs tm_eval_args(const tamcmc_ctx *c, int tiles, bool grad, double *d_logL, int32_t *d_status, const int32_t *d_rows,
                        double *d_model)
{
    TmEvalArgs a{};
    a.x2 = c->d_x2; a.y = c->d_y; a.lx = c->d_lx; a.isig2 = c->d_isig2;
    a.spec = (c->nspec > 1) ? c->d_spec : nullptr;
    a.mult = c->d_mult; a.noise = c->d_noise; a.cell = c->d_cell; a.thdr = c->d_thdr; a.tidx = c->d_tidx; a.wt = c->d_wt;
    a.part = c->d_part; a.gmult = grad ? c->d_gmult : nullptr; a.gnoise = grad ? c->d_gnoise : nullptr;
    a.row_of_chain = d_rows; a.model_out = d_model;
    a.ticket = grad ? nullptr : c->d_ticket; a.logL = d_logL; a.status = d_status;
    a.Nx = c->L.Nx; a.n_mult = c->L.n_mult; a.tiles = tiles; a.cells = c->cells; a.likelihood_case = c->L.likelihood_case;
    a.like_p = c->L.like_p;
    a.order = c->d_order; a.order_mode = (tiles <= 65535) ? c->order_mode : 0; a.prio = c->prio;
    a.generic = (c->L.likelihood_case != 0 || c->L.family == TM_FAM_GAUSS || d_rows != nullptr) ? 1 : 0;
    if (tiles == 1 && a.order_mode == 2) a.order_mode = 1;     // nothing to rank
    a.tile_magic = ((1ULL << 40) + (unsigned long long)tiles - 1) / (unsigned long long)tiles;
    return a;
}

// Enqueue setup -> eval (-> backward) for device-resident inputs on the context stream.
int tm_enqueue(tamcmc_ctx *c, int Nchains, const double *d_params, const double *d_T, double *d_logL, double *d_grad,
               int32_t *d_status, const int32_t *d_rows, double *d_model)
{
    const bool grad = d_grad != nullptr;
    const hipStream_t stream = c->stream;
    if (!tm_batch_fits(c, Nchains, grad)) return TAMCMC_E_INVALID;   // a grid the runtime would reject (tamcmc_host.h)
    TM_HIP(tm_ctx_settle(c));
    c->enq_seq++;
    // several spectra resident: every chain of the batch must have been told which one it is fitted to (a batch longer
    // than the map used to fall back to spectrum 0 for all chains -- silently the wrong data)
    if (c->nspec > 1 && (c->d_spec == nullptr || Nchains > c->spec_n)) return TAMCMC_E_INVALID;
    const int units = c->units, cells = c->cells;
    const int tiles = tm_ctx_tiles(c, grad);
    if (!grad) c->last_tiles = tiles;
    double *const p_hser = grad ? c->d_hser : nullptr;
    void *const p_chain_rec = grad ? c->d_chain_rec : nullptr;
    void *const p_aux = grad ? c->d_aux : nullptr;
    const TmEvalArgs a = tm_eval_args(c, tiles, grad, d_logL, d_status, d_rows, d_model);
    const bool fused = tm_takes_fused(c, tiles);
    int rc = 0;
    if (!fused) {
        rc = tm_launch_setup(c->L, Nchains, d_params, d_T, c->d_wt, c->d_lx, units, cells, tiles, c->equal_cost, grad ? c->cost_g : c->cost_l,
                             c->d_mult, c->d_noise, c->d_cell, c->d_thdr, c->d_tidx, p_chain_rec, p_aux,
                             p_hser, a.order_mode == 2 ? c->d_order : nullptr, stream);
        if (rc != 0) return tm_launch_failed("setup", rc);
    }
    const bool timed = c->profile && (c->profile_count++ % c->profile_stride == 0);
    if (timed) { rc = c->timer.begin(stream); if (rc != TAMCMC_OK) return rc; }
    if (fused) {
        TmFusedArgs f{};
        f.params = d_params; f.Tcoefs = d_T;
        f.chain_rec = p_chain_rec; f.aux = p_aux; f.hser = p_hser;
        f.p_doubles = (c->L.Nparams + 1) & ~1;
        rc = tm_launch_fused(c->L, f, a, Nchains, grad, stream);
    } else {
        rc = tm_launch_eval(a, Nchains, grad, stream);
    }
    if (rc != 0) {
        tm_zero_tickets(c, Nchains, stream);
        return tm_launch_failed("eval", rc);
    }
    if (timed) { rc = c->timer.end(stream); if (rc != TAMCMC_OK) return rc; }
    if (grad) {      // (without: finalize happens inside the eval launch, by the last-arriving workgroup of a chain)
        rc = tm_launch_backward(c->L, Nchains, units, cells, tiles, tm_setup_balances(units, tiles, c->equal_cost, c->cost_g.pad), c->cost_g, d_params, c->d_wt, p_chain_rec, p_aux, c->d_noise, c->d_part,
                                a.gmult, a.gnoise, c->d_cell, c->d_thdr, p_hser, c->Nvars, c->d_relax, d_grad, d_logL, d_status,
                                stream);
        if (rc != 0) return tm_launch_failed("backward", rc);
    }
    return TAMCMC_OK;
}

static int grad_supported(const tamcmc_ctx *c)
{
    if (c->Nvars <= 0 || !c->d_relax) return TAMCMC_E_NOVARS;
    return TAMCMC_OK;
}

extern "C" int tamcmc_eval_batch_device(tamcmc_ctx *c, int32_t Nchains, int32_t Nparams,
                                        const double *d_params, const double *d_Tcoefs,
                                        double *d_logL, double *d_grad, int32_t *d_status)
{
    if (!ctx_usable(c) || Nchains < 1 || !d_params || !d_Tcoefs || !d_logL) return TAMCMC_E_INVALID;
    if (Nparams != c->L.Nparams) return TAMCMC_E_INVALID;
    if (d_grad) { int rc = grad_supported(c); if (rc != TAMCMC_OK) return rc; }
    TM_HIP(hipSetDevice(c->device));
    int rc = tm_ensure_capacity(c, Nchains, d_grad != nullptr);
    if (rc != TAMCMC_OK) return rc;
    return tm_enqueue(c, Nchains, d_params, d_Tcoefs, d_logL, d_grad, d_status, nullptr, nullptr);
}

// Wait for everything enqueued so far (tm_poll_event).
static int wait_done(tamcmc_ctx *c)
{
    if (!c->ev_done) TM_HIP(hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming));
    TM_HIP(hipEventRecord(c->ev_done, c->stream));
    return tm_poll_event(c->ev_done);
}

static inline TmWatch ctx_watch(tamcmc_ctx *c)
{
    return TmWatch{c->h_out.host<uint64_t>(), c->h_status.host<int32_t>(), &c->ev_done, &c->ev_recorded, c->stream};
}
static void mark_pending(tamcmc_ctx *c, int n, size_t nw) { tm_mark_slots(ctx_watch(c), n, nw); }
static int wait_data(tamcmc_ctx *c, int n, size_t nw)
{
    return tm_wait_slots(ctx_watch(c), n, nw, [c]() { tm_zero_tickets(c, c->cap, c->stream); });
}

// What a host-pointer call needs: the per-batch device buffers, and the pinned, device-mapped staging.
static int ensure_host(tamcmc_ctx *c, int Nchains, bool grad)
{
    int rc = tm_ensure_capacity(c, Nchains, grad);
    if (rc != TAMCMC_OK || (Nchains <= c->h_cap && c->h_nvars == c->Nvars)) return rc;
    TM_HIP(tm_ctx_stream_sync(c));
    c->h_in.release(); c->h_out.release(); c->h_status.release();
    c->h_cap = 0;
    const size_t cap = (size_t)(Nchains > c->cap ? Nchains : c->cap);
    rc = c->h_in.reserve(cap * ((size_t)c->L.Nparams + 1) * sizeof(double), TM_PIN_MAPPED);
    if (rc == TAMCMC_OK) rc = c->h_out.reserve(cap * ((size_t)(c->Nvars > 0 ? c->Nvars : 0) + 1) * sizeof(double), TM_PIN_MAPPED);
    if (rc == TAMCMC_OK) rc = c->h_status.reserve(cap * sizeof(int32_t), TM_PIN_MAPPED);
    if (rc != TAMCMC_OK) return rc;
    c->h_cap = (int)cap; c->h_nvars = c->Nvars;
    return TAMCMC_OK;
}

// The launches of a batch whose inputs are (or, behind a gate, will be) in the staging: they read and write its device views.
static int enqueue_staged(tamcmc_ctx *c, int Nchains, bool grad, const int32_t *d_rows, double *d_model)
{
    const size_t n = (size_t)Nchains;
    double *const in = c->h_in.dev<double>(), *const out = c->h_out.dev<double>();
    return tm_enqueue(c, Nchains, in, in + n * c->L.Nparams, out, grad ? out + n : nullptr, c->h_status.dev<int32_t>(), d_rows, d_model);
}

extern "C" int tamcmc_eval_batch_begin(tamcmc_ctx *c, int32_t Nchains, int32_t Nparams, const double *params, const double *Tcoefs)
{
    if (!c || Nchains < 1 || !params || !Tcoefs || Nparams != c->L.Nparams || c->in_flight || c->armed) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(c->device));
    int rc = ensure_host(c, Nchains, false);
    if (rc != TAMCMC_OK) return rc;
    tm_stage_inputs(c->h_in.h, params, (size_t)Nchains * (size_t)Nparams, Tcoefs, (size_t)Nchains);
    mark_pending(c, Nchains, (size_t)Nchains);
    rc = enqueue_staged(c, Nchains, false, nullptr, nullptr);
    if (rc != TAMCMC_OK) return rc;
    c->ev_recorded = false;          // wait_data records the completion event only if the results are slow to arrive
    c->in_flight = Nchains;
    return TAMCMC_OK;
}

extern "C" int tamcmc_eval_batch_end(tamcmc_ctx *c, int32_t Nchains, double *logL, int32_t *status)
{
    if (!c || !logL || c->in_flight != Nchains) return TAMCMC_E_INVALID;
    c->in_flight = 0;
    { const int rc = wait_data(c, Nchains, (size_t)Nchains); if (rc != TAMCMC_OK) return rc; }
    std::memcpy(logL, c->h_out.h, (size_t)Nchains * sizeof(double));
    if (status) std::memcpy(status, c->h_status.h, (size_t)Nchains * sizeof(int32_t));
    return TAMCMC_OK;
}

extern "C" int tamcmc_eval_batch_poll(const tamcmc_ctx *c, int32_t chain, double *logL, int32_t *status)
{
    if (!c || !logL || !status || chain < 0 || chain >= c->in_flight) return TAMCMC_E_INVALID;
    return tm_poll_slot(c->h_out.host<uint64_t>(), c->h_status.host<int32_t>(), (size_t)chain, logL, status);
}

int tm_launch_gate(uint32_t *dv_gate, uint32_t target, int patience, void *stream);      // tamcmc_setup.hip
#define TM_GATE_EXPIRED 16
#define TM_GATE_FIRING 32

// The host's side of the gate's expiry protocol (tamcmc_setup.hip): announce, then look.  true: the gate has given up and
// the armed launches ran (or are running) on stale input -- the caller opens the word anyway, lets them drain and starts over.
static bool gate_claim(tamcmc_ctx *c)
{
    __atomic_store_n(gate_word(c) + TM_GATE_FIRING, c->gate_seq, __ATOMIC_SEQ_CST);
    return __atomic_load_n(gate_word(c) + TM_GATE_EXPIRED, __ATOMIC_SEQ_CST) == c->gate_seq;
}

// An armed batch: its launches are put into the stream AHEAD of its parameters, behind a one-wave gate kernel that
// watches a pinned word.  A host loop arms batch i+1 while the GPU evaluates batch i (the launch calls, ~6 us, are then
// hidden under that evaluation) and fires it with one store once the parameters are known.
extern "C" int tamcmc_eval_batch_arm(tamcmc_ctx *c, int32_t Nchains)
{
    if (!c || Nchains < 1 || c->armed) return TAMCMC_E_INVALID;
    if (c->in_flight && c->in_flight != Nchains) return TAMCMC_E_INVALID;
    // never (re)allocate under a batch in flight: tamcmc_ctx_reserve (or an earlier batch of this size) sized the buffers
    if (Nchains > c->cap || Nchains > c->h_cap || c->h_nvars != c->Nvars) {
        if (c->in_flight) return TAMCMC_E_INVALID;
        const int rc = tamcmc_ctx_reserve(c, Nchains);
        if (rc != TAMCMC_OK) return rc;
    }
    TM_HIP(hipSetDevice(c->device));
    if (!c->gate.fits(256)) {
        const int rc = c->gate.reserve(256, TM_PIN_MAPPED);
        if (rc != TAMCMC_OK) return rc;
        std::memset(c->gate.h, 0, 256);
        c->gate_seq = 1;               // (0 is what the expiry / firing words hold before the first batch)
        *gate_word(c) = c->gate_seq;
    }
    const uint32_t target = c->gate_seq + 1;
    TM_HIP(tm_ctx_settle(c));
    c->enq_seq++;
    int rc = tm_launch_gate(c->gate.dev<uint32_t>(), target, c->gate_patience, c->stream);
    if (rc != 0) return tm_launch_failed("gate", rc);
    rc = enqueue_staged(c, Nchains, false, nullptr, nullptr);
    c->gate_seq = target;
    if (rc != TAMCMC_OK) {            // the gate is in the stream: open it, nothing sits behind it
        __atomic_store_n(gate_word(c), target, __ATOMIC_RELEASE);
        return rc;
    }
    c->armed = Nchains;
    return TAMCMC_OK;
}

extern "C" int tamcmc_eval_batch_fire(tamcmc_ctx *c, int32_t Nchains, int32_t Nparams, const double *params, const double *Tcoefs)
{
    if (!c || !params || !Tcoefs || Nparams != c->L.Nparams || c->armed != Nchains || Nchains < 1 || c->in_flight) return TAMCMC_E_INVALID;
    if (gate_claim(c)) {
        // the gate gave up waiting (the host was held up for seconds): the armed launches used stale input.  Let them
        // drain and evaluate this batch the plain way.
        __atomic_store_n(gate_word(c), c->gate_seq, __ATOMIC_RELEASE);
        c->armed = 0;
        TM_HIP(tm_ctx_stream_sync(c));
        return tamcmc_eval_batch_begin(c, Nchains, Nparams, params, Tcoefs);
    }
    tm_stage_inputs(c->h_in.h, params, (size_t)Nchains * (size_t)Nparams, Tcoefs, (size_t)Nchains);
    mark_pending(c, Nchains, (size_t)Nchains);
    __atomic_store_n(gate_word(c), c->gate_seq, __ATOMIC_RELEASE);      // (after the parameters and the markers)
    c->ev_recorded = false;
    c->armed = 0;
    c->in_flight = Nchains;
    return TAMCMC_OK;
}

// Opens the gate of an armed batch that will not be fired (the loop ended, or failed): it runs on whatever the input
// buffer holds -- the previous batch's parameters -- and is waited for here; nothing is handed out.
extern "C" int tamcmc_eval_batch_disarm(tamcmc_ctx *c)
{
    if (!c) return TAMCMC_E_INVALID;
    if (!c->armed) return TAMCMC_OK;
    if (c->in_flight) return TAMCMC_E_INVALID;        // collect the batch in flight first (_end)
    const int n = c->armed;
    if (gate_claim(c)) {              // it has run (or is running) already: just let it retire
        __atomic_store_n(gate_word(c), c->gate_seq, __ATOMIC_RELEASE);
        c->armed = 0;
        TM_HIP(tm_ctx_stream_sync(c));
        return TAMCMC_OK;
    }
    mark_pending(c, n, (size_t)n);
    __atomic_store_n(gate_word(c), c->gate_seq, __ATOMIC_RELEASE);
    c->ev_recorded = false;
    c->armed = 0;
    return wait_data(c, n, (size_t)n);
}

extern "C" int tamcmc_ctx_reserve(tamcmc_ctx *c, int32_t Nchains)
{
    if (!c || Nchains < 1 || c->in_flight || c->armed) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(c->device));
    return ensure_host(c, Nchains, false);
}

extern "C" int tamcmc_eval_batch(tamcmc_ctx *c, int32_t Nchains, int32_t Nparams,
                                 const double *params, const double *Tcoefs,
                                 double *logL, double *grad,
                                 int32_t n_rows, const int32_t *model_rows, double *model_out,
                                 int32_t *status)
{
    if (!c || Nchains < 1 || !params || !Tcoefs || !logL) return TAMCMC_E_INVALID;
    if (Nparams != c->L.Nparams) return TAMCMC_E_INVALID;
    if (n_rows < 0 || (n_rows > 0 && (!model_rows || !model_out))) return TAMCMC_E_INVALID;
    for (int r = 0; r < n_rows; r++)
        if (model_rows[r] < 0 || model_rows[r] >= Nchains) return TAMCMC_E_INVALID;
    if (grad) { int rc = grad_supported(c); if (rc != TAMCMC_OK) return rc; }
    if (c->in_flight || c->armed) return TAMCMC_E_INVALID;   // (buffers may move below)
    TM_HIP(hipSetDevice(c->device));
    int rc = ensure_host(c, Nchains, grad != nullptr);
    if (rc != TAMCMC_OK) return rc;
    const size_t n = (size_t)Nchains;
    tm_stage_inputs(c->h_in.h, params, (size_t)Nchains * (size_t)Nparams, Tcoefs, (size_t)Nchains);
    const int32_t *d_rows = nullptr;
    if (n_rows > 0) {
        std::vector<int32_t> rows(n, -1);
        for (int r = 0; r < n_rows; r++) rows[(size_t)model_rows[r]] = r;   // a chain listed twice keeps the last row
        const size_t need = (size_t)n_rows * (size_t)c->L.Nx;
        if (need > c->model_cap) {
            TM_HIP(tm_ctx_stream_sync(c));
            (void)hipFree(c->d_model); c->d_model = nullptr; c->model_cap = 0;
            TM_HIP(hipMalloc(&c->d_model, need * sizeof(double)));
            c->model_cap = need;
        }
        TM_HIP(hipMemcpyAsync(c->d_rows, rows.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        TM_HIP(tm_ctx_stream_sync(c));   // rows is a local
        d_rows = c->d_rows;
    }
    // logL / status (a few hundred bytes) are written straight into the mapped host buffer by the last kernel; the
    // the backward kernel writes each chain's gradient row as one run of consecutive stores, straight into the mapped
    // host buffer (a copy-engine transfer of these ~20 KB would add ~20 us of latency)
    const bool watch = (n_rows == 0);                         // no model rows to copy back: watch the results arrive (wait_data)
    const size_t nwatch = n * (grad ? (size_t)c->Nvars + 1 : 1);
    if (watch) mark_pending(c, Nchains, nwatch);
    rc = enqueue_staged(c, Nchains, grad != nullptr, d_rows, c->d_model);
    if (rc != TAMCMC_OK) return rc;
    if (n_rows > 0) {
        // rows whose chain was listed more than once share one device row
        for (int r = 0; r < n_rows; r++) {
            int src = r;
            for (int r2 = n_rows - 1; r2 > r; r2--) if (model_rows[r2] == model_rows[r]) { src = r2; break; }
            TM_HIP(hipMemcpyAsync(model_out + (size_t)r * c->L.Nx, c->d_model + (size_t)src * c->L.Nx,
                                  (size_t)c->L.Nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        }
    }
    if (watch) {
        c->ev_recorded = false;
        rc = wait_data(c, Nchains, nwatch);
    } else {
        rc = wait_done(c);
    }
    if (rc != TAMCMC_OK) return rc;
    TM_HIP(hipGetLastError());
    std::memcpy(logL, c->h_out.h, n * sizeof(double));
    if (status) std::memcpy(status, c->h_status.h, n * sizeof(int32_t));
    if (grad) std::memcpy(grad, c->h_out.host<double>() + n, n * (size_t)c->Nvars * sizeof(double));
    return TAMCMC_OK;
}

extern "C" int tamcmc_model_explicit(tamcmc_ctx *c, int32_t Nparams, const double *params, double *model_out, int32_t *status)
{
    if (!c || !params || !model_out) return TAMCMC_E_INVALID;
    const double T = 1.0;
    double logL = 0.0;
    const int32_t row = 0;
    int32_t st = 0;
    int rc = tamcmc_eval_batch(c, 1, Nparams, params, &T, &logL, nullptr, 1, &row, model_out, &st);
    if (status) *status = st;
    return rc;
}

extern "C" const char *tamcmc_strerror(int code)
{
    switch (code) {
    case TAMCMC_OK: return "ok";
    case TAMCMC_E_INVALID: return "invalid argument";
    case TAMCMC_E_NODEVICE: return "no usable HIP device (this library has no CPU fallback)";
    case TAMCMC_E_HIP: return "HIP runtime error (see tamcmc_last_hip_error)";
    case TAMCMC_E_MODEL_DISABLED: return "model id disabled in the reference (ids 4, 5)";
    case TAMCMC_E_UNKNOWN_MODEL: return "unknown model or likelihood id";
    case TAMCMC_E_NOMEM: return "out of memory";
    case TAMCMC_E_NOVARS: return "gradient requested before tamcmc_ctx_set_vars";
    case TAMCMC_E_NOGRAD: return "gradient not available for this model (or for so many multiplets and variables)";
    default: return "unknown error code";
    }
}

extern "C" const char *tamcmc_last_hip_error(void) { return tm_hip_err; }
#ifndef TM_KERNEL_HASH
#define TM_KERNEL_HASH "unknown"
#endif
extern "C" const char *tamcmc_version(void) { return "tamcmc_accel 0.3 (gfx950) kernels:" TM_KERNEL_HASH; }
