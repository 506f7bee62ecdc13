// tamcmc_api.cpp -- host side of the C ABI declared in include/tamcmc_accel.h.
// Owns the device buffers of one context, validates arguments the way Model_def's callers rely on
// (plength sums to Nparams, model / likelihood ids from the *.list tables), and strings the launches of
// one evaluation on the context stream:
//     setup (params -> multiplet table, tile descriptors)
//     -> eval (model + likelihood; the last workgroup of a chain sums its tiles in fixed order: -p(..)/T)
//     or eval<grad> (+ gradient partials) -> backward (tile sums, chain rule to d/dvars, logL)
// No CPU fallback exists in this library.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "tamcmc_accel.h"
#include "tamcmc_dev.h"
#include "tamcmc_group.h"
#include "tamcmc_summary.h"

static thread_local char g_hip_err[256] = "";

#define TM_HIP(call)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            snprintf(g_hip_err, sizeof(g_hip_err), "%s -> %s", #call, hipGetErrorString(e_)); \
            return TAMCMC_E_HIP;                                                             \
        }                                                                                    \
    } while (0)

struct tamcmc_ctx {
    int device = 0;
    TmLayout L{};
    // Geometry (tamcmc_dev.h): units of 512 bins, cells of 8 units, tiles_l / tiles_g tiles per chain for the likelihood-only
    // and the gradient launch -- functions of the grid alone; a chain's tile BOUNDARIES are chosen by the setup kernel.
    int units = 0, cells = 0;
    int tiles_l = 1, tiles_g = 1;
    int tiles_max = 1;
    int equal_cost = 0;            // TAMCMC_EQUAL_COST=1: per-chain tile boundaries of equal cost instead of equal length
    int prio = 0;                  // TAMCMC_PRIO=1: issue priority by launch rank (s_setprio)
    TmCostModel cost_l{60, 5, 9, TM_TILE_MAXU_L}, cost_g{110, 13, 24, TM_TILE_MAXU};   // (.pad = units per tile at most)   // VALU instructions per bin: c0 + sum(a * ncomp + b) (TAMCMC_COST / TAMCMC_COST_GRAD)
    int last_tiles = 0;            // T of the most recent likelihood-only call (tamcmc_ctx_geometry)
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // resident data
    double *d_x2 = nullptr, *d_y = nullptr, *d_lx = nullptr, *d_isig2 = nullptr;   // 2 x, y, log x, 1 / sigma^2
    int nspec = 1;                 // spectra resident in d_y / d_isig2 (blocks of Nx); tamcmc_ctx_set_spectra
    int32_t *d_spec = nullptr;     // [spec_n] chain -> spectrum map (tamcmc_ctx_set_chain_spectrum), or NULL: all chains use spectrum 0
    int spec_n = 0;
    // per-batch buffers (capacity in chains)
    int cap = 0;
    bool cap_grad = false;
    void *d_slab = nullptr;        // one allocation behind every per-batch buffer below (ensure_capacity)
    double *d_params = nullptr, *d_T = nullptr, *d_logL = nullptr, *d_part = nullptr;
    double *d_gmult = nullptr, *d_gnoise = nullptr, *d_hser = nullptr;
    int32_t *d_order = nullptr; int order_mode = 2;
    int fuse = 1;                  // one tile per chain -> prologue and evaluation in one launch (TAMCMC_FUSED=0 disables)
    int32_t *d_status = nullptr, *d_rows = nullptr;
    TmMult *d_mult = nullptr;
    TmNoise *d_noise = nullptr;
    void *d_chain_rec = nullptr, *d_aux = nullptr;   // TmChain / TmMultFull records kept for the backward kernel
    double *d_wt = nullptr;        // [cap][2] {T, wscale} device copies written by the setup kernel
    int32_t *d_ticket = nullptr;   // [cap] arrival counters of the in-launch finalize (kept at zero between launches)
    TmCellRec *d_cell = nullptr;   // [cap][cells] background polynomials
    TmTileHdr *d_thdr = nullptr;   // [cap][tiles_max] tile headers (per-chain boundaries)
    TmActive *d_tidx = nullptr;    // [cap][tiles_max][n_mult] active multiplet lists
    double *d_model = nullptr;
    size_t model_cap = 0;
    // host-pointer entry point: pinned, device-mapped staging the kernels read / write directly over PCIe
    // (no copy-engine round trips): h_in = [params | Tcoefs], h_out = [logL | grad], h_status
    double *h_in = nullptr, *h_out = nullptr;
    int32_t *h_status = nullptr;
    int h_cap = 0, h_nvars = -1;
    double *dv_in = nullptr, *dv_out = nullptr;   // device views of h_in / h_out / h_status (looked up once per allocation)
    int32_t *dv_status = nullptr;
    hipEvent_t ev_done = nullptr;  // completion of a host-pointer call, polled (see wait_done)
    bool ev_recorded = false;      // wait_data: the event of the current call has been recorded (lazily)
    int in_flight = 0;             // chains of a tamcmc_eval_batch_begin not yet collected by _end
    int armed = 0;                 // chains of a tamcmc_eval_batch_arm whose launches wait behind the gate for _fire
    uint32_t *h_gate = nullptr, *dv_gate = nullptr;   // pinned word the gate kernel watches
    uint32_t gate_seq = 0;         // value that opens the gate of the armed batch
    int gate_patience = 1 << 21;   // polls (~2 us each) before the gate gives up; TAMCMC_GATE_PATIENCE (tests)
    // variables
    int Nvars = 0;
    int32_t *d_relax = nullptr;
    // shader-clock probe (tamcmc_ctx_clock_probe_begin / _end): one wave on its own stream beside the evaluation
    hipStream_t probe_stream = nullptr;
    unsigned long long *h_probe = nullptr, *dv_probe = nullptr;   // pinned: {core cycles, 100 MHz ticks}
    // profiling
    bool profile = false;
    int profile_stride = 1;       // events around every n-th eval launch (tamcmc_ctx_profile(ctx, n))
    long long profile_count = 0;
    std::vector<hipEvent_t> ev;   // pairs (start, stop)
    size_t ev_used = 0;
    int groups = 0;               // fit groups this context is a member of (tamcmc_group_create); destroy is refused meanwhile
    int summaries = 0;            // summary objects bound to this context (tamcmc_summary_create); destroy is refused meanwhile
    // ordering against fit groups (tamcmc_group_eval_begin): enq_seq counts what this library put on the stream, so that a
    // group can tell whether anything came since it last ordered itself against it; after_ev is a group's "launches done"
    // event this stream has still to wait for -- the wait is enqueued by the next use of the stream (ctx_settle), not by
    // the group call
    uint64_t enq_seq = 0;
    hipEvent_t after_ev = nullptr;
    const void *after_owner = nullptr;
};

// A group call left an event for this stream to wait for: enqueue the wait now (before anything else goes on the stream).
static inline hipError_t ctx_settle(tamcmc_ctx *c)
{
    if (!c->after_ev) return hipSuccess;
    const hipEvent_t e = c->after_ev;
    c->after_ev = nullptr; c->after_owner = nullptr;
    return hipStreamWaitEvent(c->stream, e, 0);
}
static inline hipError_t ctx_stream_sync(tamcmc_ctx *c)
{
    const hipError_t e = ctx_settle(c);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(c->stream);
}

static int pick_tiles(const tamcmc_ctx *c, int Nchains, bool grad);

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

static int ensure_capacity(tamcmc_ctx *c, int Nchains, bool grad)
{
    if (Nchains <= c->cap && (!grad || c->cap_grad)) return TAMCMC_OK;
    const int cap = Nchains > c->cap ? Nchains : c->cap;
    const bool g = grad || c->cap_grad;
    TM_HIP(ctx_stream_sync(c));
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
    (void)hipSetDevice(c->device);
    if (c->armed && c->h_gate) { __atomic_store_n(c->h_gate, c->gate_seq, __ATOMIC_RELEASE); c->armed = 0; }   // let the gate go
    if (c->stream) (void)ctx_stream_sync(c);
    free_batch(c);
    (void)hipHostFree(c->h_gate);
    (void)hipFree(c->d_x2); (void)hipFree(c->d_y); (void)hipFree(c->d_lx); (void)hipFree(c->d_isig2); (void)hipFree(c->d_spec);
    (void)hipFree(c->d_model); (void)hipFree(c->d_relax);
    (void)hipHostFree(c->h_in); (void)hipHostFree(c->h_out); (void)hipHostFree(c->h_status);
    if (c->probe_stream) { (void)hipStreamSynchronize(c->probe_stream); (void)hipStreamDestroy(c->probe_stream); }
    (void)hipHostFree(c->h_probe);
    if (c->ev_done) (void)hipEventDestroy(c->ev_done);
    for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return TAMCMC_OK;
}

extern "C" int tamcmc_ctx_set_vars(tamcmc_ctx *c, int32_t Nvars, const int32_t *index_to_relax)
{
    if (c && c->armed) return TAMCMC_E_INVALID;     // launches wait behind a gate: only _fire / _end / _disarm / destroy (tamcmc_accel.h)
    if (!c || Nvars < 0 || (Nvars > 0 && !index_to_relax)) return TAMCMC_E_INVALID;
    for (int i = 0; i < Nvars; i++)
        if (index_to_relax[i] < 0 || index_to_relax[i] >= c->L.Nparams) return TAMCMC_E_INVALID;
    // a layout whose gradient tables outgrow the backward kernel's LDS (every entry a variable: from some 210 to 235 multiplets on)
    // is refused here, the context left as it was -- not at the first gradient batch, after two of its three launches
    if (Nvars > 0 && !tm_backward_fits(c->L, c->tiles_g, Nvars)) return TAMCMC_E_NOGRAD;
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(ctx_stream_sync(c));
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
    if (c && c->armed) return TAMCMC_E_INVALID;     // launches wait behind a gate: only _fire / _end / _disarm / destroy (tamcmc_accel.h)
    if (!c || Nspectra < 1 || !y || (c->L.likelihood_case == 1 && !sigma_y)) return TAMCMC_E_INVALID;
    if (c->summaries > 0) return TAMCMC_E_INVALID;  // a summary's running state belongs to the resident spectrum
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(ctx_stream_sync(c));
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
    if (c && c->armed) return TAMCMC_E_INVALID;     // launches wait behind a gate: only _fire / _end / _disarm / destroy (tamcmc_accel.h)
    if (!c || Nchains < 0 || (Nchains > 0 && !spectrum_of_chain)) return TAMCMC_E_INVALID;
    for (int m = 0; m < Nchains; m++)
        if (spectrum_of_chain[m] < 0 || spectrum_of_chain[m] >= c->nspec) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(ctx_stream_sync(c));
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
    if (c && c->armed) return TAMCMC_E_INVALID;     // launches wait behind a gate: only _fire / _end / _disarm / destroy (tamcmc_accel.h)
    if (!c) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(ctx_stream_sync(c));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    c->enq_seq++;
    return TAMCMC_OK;
}

extern "C" int tamcmc_ctx_synchronize(tamcmc_ctx *c)
{
    if (c && c->armed) return TAMCMC_E_INVALID;     // launches wait behind a gate: only _fire / _end / _disarm / destroy (tamcmc_accel.h)
    if (!c) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(ctx_stream_sync(c));
    return TAMCMC_OK;
}

extern "C" int tamcmc_ctx_profile(tamcmc_ctx *c, int enable)
{
    if (!c) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(ctx_stream_sync(c));
    c->profile = enable != 0;
    c->profile_stride = enable > 1 ? enable : 1;
    c->profile_count = 0;
    c->ev_used = 0;
    // a pool of events up front: creating one costs ~10 us, which would land inside the caller's timed region
    while (c->profile && c->ev.size() < 256) {
        hipEvent_t e;
        TM_HIP(hipEventCreate(&e));
        c->ev.push_back(e);
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_ctx_kernel_time(tamcmc_ctx *c, double *total_ms, int64_t *launches)
{
    if (c && c->armed) return TAMCMC_E_INVALID;     // launches wait behind a gate: only _fire / _end / _disarm / destroy (tamcmc_accel.h)
    if (!c || !total_ms || !launches) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(ctx_stream_sync(c));
    double t = 0.0;
    for (size_t i = 0; i + 1 < c->ev_used; i += 2) {
        float ms = 0.f;
        TM_HIP(hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]));
        t += (double)ms;
    }
    *total_ms = t;
    *launches = (int64_t)(c->ev_used / 2);
    return TAMCMC_OK;
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
    if (!c->h_probe) {
        TM_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->h_probe), 2 * sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent));
        TM_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&c->dv_probe), c->h_probe, 0));
    }
    c->h_probe[0] = c->h_probe[1] = 0;
    hipLaunchKernelGGL(tamcmc_clock_probe_kernel, dim3(1), dim3(64), 0, c->probe_stream,
                       (unsigned long long)(milliseconds * 1e5), c->dv_probe);
    TM_HIP(hipGetLastError());
    return TAMCMC_OK;
}

extern "C" int tamcmc_ctx_clock_probe_end(tamcmc_ctx *c, double *core_GHz, double *seconds)
{
    if (!c || !c->probe_stream || !core_GHz) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(hipStreamSynchronize(c->probe_stream));
    const double cyc = (double)c->h_probe[0], t = (double)c->h_probe[1] / 1e8;
    *core_GHz = (t > 0.0) ? cyc / t / 1e9 : 0.0;
    if (seconds) *seconds = t;
    return TAMCMC_OK;
}

extern "C" int tamcmc_ctx_geometry(tamcmc_ctx *c, int32_t *bins_per_tile, int32_t *tiles, int32_t *threads_per_block,
                                   int32_t *n_multiplets)
{
    if (!c) return TAMCMC_E_INVALID;
    const int T = c->last_tiles > 0 ? c->last_tiles : pick_tiles(c, 64, false);
    if (bins_per_tile) *bins_per_tile = TM_UNIT_BINS * c->cost_l.pad;   // largest tile of the likelihood launch (TM_TILE_MAXU_L units; TM_TILE_MAXU when balanced, and always for the gradient launch)
    if (tiles) *tiles = T;
    if (threads_per_block) *threads_per_block = TM_THREADS;
    if (n_multiplets) *n_multiplets = c->L.n_mult;
    return TAMCMC_OK;
}

// Number of tiles.  It depends on the grid only, never on the batch: a chain's result must not change with the number
// of chains evaluated beside it (a sharded run and a single-process run have to produce bit-identical chains).
static int pick_tiles(const tamcmc_ctx *c, int /*Nchains*/, bool grad)
{
    return grad ? c->tiles_g : c->tiles_l;
}

// Arguments of the eval launch of a batch on the context (solo launches and fit groups alike).
static TmEvalArgs eval_args(const tamcmc_ctx *c, int tiles, bool grad, double *d_logL, int32_t *d_status, const int32_t *d_rows,
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

// one tile per chain (short grids): prologue and evaluation share a launch (TAMCMC_TILES=1 on a 9..16-unit grid: two launches)
static bool takes_fused(const tamcmc_ctx *c, int tiles) { return tiles == 1 && c->fuse != 0 && c->units <= TM_TILE_MAXU; }

// Enqueue setup -> eval (-> backward) for device-resident inputs on the context stream.
static int enqueue(tamcmc_ctx *c, int Nchains, const double *d_params, const double *d_T, double *d_logL,
                   double *d_grad, int32_t *d_status, const int32_t *d_rows, double *d_model)
{
    const bool grad = d_grad != nullptr;
    const hipStream_t stream = c->stream;
    TM_HIP(ctx_settle(c));
    c->enq_seq++;
    // several spectra resident: every chain of the batch must have been told which one it is fitted to (a batch longer
    // than the map used to fall back to spectrum 0 for all chains -- silently the wrong data)
    if (c->nspec > 1 && (c->d_spec == nullptr || Nchains > c->spec_n)) return TAMCMC_E_INVALID;
    const int units = c->units, cells = c->cells;
    const int tiles = pick_tiles(c, Nchains, grad);
    if (!grad) c->last_tiles = tiles;
    double *const p_hser = grad ? c->d_hser : nullptr;
    void *const p_chain_rec = grad ? c->d_chain_rec : nullptr;
    void *const p_aux = grad ? c->d_aux : nullptr;
    const TmEvalArgs a = eval_args(c, tiles, grad, d_logL, d_status, d_rows, d_model);
    const bool fused = takes_fused(c, tiles);
    int rc = 0;
    if (!fused) {
        rc = tm_launch_setup(c->L, Nchains, d_params, d_T, c->d_wt, c->d_lx, units, cells, tiles, c->equal_cost, grad ? c->cost_g : c->cost_l,
                             c->d_mult, c->d_noise, c->d_cell, c->d_thdr, c->d_tidx, p_chain_rec, p_aux,
                             p_hser, a.order_mode == 2 ? c->d_order : nullptr, stream);
        if (rc != 0) { snprintf(g_hip_err, sizeof(g_hip_err), "setup launch -> %s", hipGetErrorString((hipError_t)rc)); return TAMCMC_E_HIP; }
    }
    const bool timed = c->profile && (c->profile_count++ % c->profile_stride == 0);
    if (timed) {
        while (c->ev.size() < c->ev_used + 2) {
            hipEvent_t e;
            TM_HIP(hipEventCreate(&e));
            c->ev.push_back(e);
        }
        TM_HIP(hipEventRecord(c->ev[c->ev_used], stream));
    }
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
        snprintf(g_hip_err, sizeof(g_hip_err), "eval launch -> %s", hipGetErrorString((hipError_t)rc));
        (void)hipMemsetAsync(c->d_ticket, 0, (size_t)Nchains * sizeof(int32_t), stream);   // arrival counters back to zero
        return TAMCMC_E_HIP;
    }
    if (timed) {
        TM_HIP(hipEventRecord(c->ev[c->ev_used + 1], stream));
        c->ev_used += 2;
    }
    if (!grad) {
        // finalize happens inside the eval launch (last-arriving workgroup per chain)
    } else {
        rc = tm_launch_backward(c->L, Nchains, units, cells, tiles, tm_setup_balances(units, tiles, c->equal_cost, (grad ? c->cost_g : c->cost_l).pad), c->cost_g, d_params, c->d_wt, p_chain_rec, p_aux, c->d_noise, c->d_part,
                                a.gmult, a.gnoise, c->d_cell, c->d_thdr, p_hser, c->Nvars, c->d_relax, d_grad, d_logL, d_status,
                                stream);
        if (rc != 0) { snprintf(g_hip_err, sizeof(g_hip_err), "backward launch -> %s", hipGetErrorString((hipError_t)rc)); return TAMCMC_E_HIP; }
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
    if (c && c->armed) return TAMCMC_E_INVALID;     // launches wait behind a gate: only _fire / _end / _disarm / destroy (tamcmc_accel.h)
    if (!c || Nchains < 1 || !d_params || !d_Tcoefs || !d_logL) return TAMCMC_E_INVALID;
    if (Nparams != c->L.Nparams) return TAMCMC_E_INVALID;
    if (d_grad) { int rc = grad_supported(c); if (rc != TAMCMC_OK) return rc; }
    TM_HIP(hipSetDevice(c->device));
    int rc = ensure_capacity(c, Nchains, d_grad != nullptr);
    if (rc != TAMCMC_OK) return rc;
    return enqueue(c, Nchains, d_params, d_Tcoefs, d_logL, d_grad, d_status, nullptr, nullptr);
}

// Wait for everything enqueued so far by polling an event.  hipStreamSynchronize may park the calling thread on an
// interrupt; on this platform that path showed rare stalls of 1-40 ms after a ~160 us batch (profiles/README.md),
// and a sampler calls this thousands of times per second.
static int wait_done(tamcmc_ctx *c)
{
    if (!c->ev_done) TM_HIP(hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming));
    TM_HIP(hipEventRecord(c->ev_done, c->stream));
    for (;;) {
        const hipError_t e = hipEventQuery(c->ev_done);
        if (e == hipSuccess) return TAMCMC_OK;
        if (e != hipErrorNotReady) { snprintf(g_hip_err, sizeof(g_hip_err), "hipEventQuery -> %s", hipGetErrorString(e)); return TAMCMC_E_HIP; }
        __builtin_ia32_pause();
    }
}

// Host path without model rows: instead of waiting for the launch to retire, watch the results arrive.  Every logL and
// gradient entry is one aligned 8-byte store and every status one 4-byte store into coherent pinned memory, written
// exactly once per launch, so a slot that no longer holds the marker put there before the launch holds its final
// value -- no ordering between slots is assumed.  The completion event is still recorded and consulted now and then:
// a failed launch ends the wait with an error instead of a hang, and should a result ever equal the marker (a kernel
// NaN does not have this payload) the wait ends when the launch retires.
static const uint64_t TM_PENDING_BITS = 0x7FF8DEADBEEF5A5AULL;
// The marker / wait code, shared by a context's host path and a fit group's (tamcmc_group_eval_begin): out = the watched
// doubles (the first n of them are the logL slots), st = the n status slots, ev / recorded = the completion event of the
// call, recorded lazily on `stream`.
struct TmWatch {
    uint64_t *out;
    int32_t *st;
    hipEvent_t *ev;
    bool *recorded;
    hipStream_t stream;
};
// nw = doubles to watch: n (logL) or n * (1 + Nvars) (logL, then the gradient rows)
static void mark_slots(const TmWatch &w, int n, size_t nw)
{
    for (size_t m = 0; m < nw; m++) w.out[m] = TM_PENDING_BITS;
    for (int m = 0; m < n; m++) w.st[m] = -1;
}
// rearm(): puts the arrival counters behind the watched launch back to zero (called on every error path)
template <class Rearm>
static int wait_slots(const TmWatch &w, int n, size_t nw, Rearm rearm)
{
    volatile const uint64_t *o = w.out;
    volatile const int32_t *st = w.st;
    unsigned spins = 0;
    for (size_t m = 0; m < nw;) {
        if (o[m] != TM_PENDING_BITS && (m >= (size_t)n || st[m] != -1)) { m++; continue; }
        __builtin_ia32_pause();
        if ((++spins & 2047u) == 0) {
            // The completion event is recorded only now, behind the kernels already in the stream (it completes once they
            // have): a call that gets its results within the first ~2000 polls -- every healthy call -- never pays for an
            // event on the launch path (~1.5 us of host time per call in a sampler loop).
            if (!*w.recorded) {
                if (!*w.ev && hipEventCreateWithFlags(w.ev, hipEventDisableTiming) != hipSuccess) return TAMCMC_E_HIP;
                if (hipEventRecord(*w.ev, w.stream) != hipSuccess) return TAMCMC_E_HIP;
                *w.recorded = true;
            }
            const hipError_t e = hipEventQuery(*w.ev);
            if (e == hipSuccess) {
                // The launch has retired: whatever the slots hold is final.  A logL / status slot that still holds its
                // marker was never written -- a chain whose finalize did not run (e.g. an arrival counter left non-zero
                // by an earlier failed launch).  Report it instead of handing the marker out as a result, and re-arm
                // the counters so that the context is usable again.
                for (size_t k = 0; k < (size_t)n; k++)
                    if (o[k] == TM_PENDING_BITS || st[k] == -1) {
                        snprintf(g_hip_err, sizeof(g_hip_err), "chain %zu was not finalized by a retired launch", k);
                        rearm();
                        return TAMCMC_E_HIP;
                    }
                return TAMCMC_OK;
            }
            if (e != hipErrorNotReady) {
                snprintf(g_hip_err, sizeof(g_hip_err), "hipEventQuery -> %s", hipGetErrorString(e));
                rearm();
                return TAMCMC_E_HIP;
            }
        }
    }
    return TAMCMC_OK;
}
// one slot: TAMCMC_PENDING, or its final value
static inline int poll_slot(const uint64_t *out, const int32_t *status, size_t slot, double *logL, int32_t *st_out)
{
    const uint64_t v = reinterpret_cast<volatile const uint64_t *>(out)[slot];
    const int32_t st = reinterpret_cast<volatile const int32_t *>(status)[slot];
    if (v == TM_PENDING_BITS || st == -1) return TAMCMC_PENDING;
    std::memcpy(logL, &v, sizeof(double));
    *st_out = st;
    return TAMCMC_OK;
}

static inline TmWatch ctx_watch(tamcmc_ctx *c)
{
    return TmWatch{reinterpret_cast<uint64_t *>(c->h_out), c->h_status, &c->ev_done, &c->ev_recorded, c->stream};
}
static void mark_pending(tamcmc_ctx *c, int n, size_t nw) { mark_slots(ctx_watch(c), n, nw); }
static int wait_data(tamcmc_ctx *c, int n, size_t nw)
{
    return wait_slots(ctx_watch(c), n, nw, [c]() { (void)hipMemsetAsync(c->d_ticket, 0, (size_t)c->cap * sizeof(int32_t), c->stream); });
}

// pinned, device-mapped staging of the host-pointer entry points
static int ensure_staging(tamcmc_ctx *c, int Nchains)
{
    const int Nparams = c->L.Nparams;
    if (Nchains <= c->h_cap && c->h_nvars == c->Nvars) return TAMCMC_OK;
    TM_HIP(ctx_stream_sync(c));
    (void)hipHostFree(c->h_in); (void)hipHostFree(c->h_out); (void)hipHostFree(c->h_status);
    c->h_in = c->h_out = nullptr; c->h_status = nullptr; c->h_cap = 0;
    const unsigned flags = hipHostMallocMapped | hipHostMallocCoherent;
    const size_t cap = (size_t)(Nchains > c->cap ? Nchains : c->cap);
    TM_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->h_in), cap * ((size_t)Nparams + 1) * sizeof(double), flags));
    TM_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->h_out), cap * ((size_t)(c->Nvars > 0 ? c->Nvars : 0) + 1) * sizeof(double), flags));
    TM_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->h_status), cap * sizeof(int32_t), flags));
    TM_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&c->dv_in), c->h_in, 0));
    TM_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&c->dv_out), c->h_out, 0));
    TM_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&c->dv_status), c->h_status, 0));
    c->h_cap = (int)cap; c->h_nvars = c->Nvars;
    return TAMCMC_OK;
}

extern "C" int tamcmc_eval_batch_begin(tamcmc_ctx *c, int32_t Nchains, int32_t Nparams, const double *params, const double *Tcoefs)
{
    if (!c || Nchains < 1 || !params || !Tcoefs || Nparams != c->L.Nparams || c->in_flight || c->armed) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(c->device));
    int rc = ensure_capacity(c, Nchains, false);
    if (rc != TAMCMC_OK) return rc;
    rc = ensure_staging(c, Nchains);
    if (rc != TAMCMC_OK) return rc;
    const size_t n = (size_t)Nchains;
    std::memcpy(c->h_in, params, n * Nparams * sizeof(double));
    std::memcpy(c->h_in + n * Nparams, Tcoefs, n * sizeof(double));
    double *dv_in = nullptr, *dv_out = nullptr;
    int32_t *dv_status = nullptr;
    dv_in = c->dv_in; dv_out = c->dv_out; dv_status = c->dv_status;
    mark_pending(c, Nchains, (size_t)Nchains);
    rc = enqueue(c, Nchains, dv_in, dv_in + n * Nparams, dv_out, nullptr, dv_status, nullptr, nullptr);
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
    std::memcpy(logL, c->h_out, (size_t)Nchains * sizeof(double));
    if (status) std::memcpy(status, c->h_status, (size_t)Nchains * sizeof(int32_t));
    return TAMCMC_OK;
}

extern "C" int tamcmc_eval_batch_poll(const tamcmc_ctx *c, int32_t chain, double *logL, int32_t *status)
{
    if (!c || !logL || !status || chain < 0 || chain >= c->in_flight) return TAMCMC_E_INVALID;
    return poll_slot(reinterpret_cast<const uint64_t *>(c->h_out), c->h_status, (size_t)chain, logL, status);
}

int tm_launch_gate(uint32_t *dv_gate, uint32_t target, int patience, void *stream);      // tamcmc_setup.hip
#define TM_GATE_EXPIRED 16
#define TM_GATE_FIRING 32

// The host's side of the gate's expiry protocol (tamcmc_setup.hip): announce, then look.  true: the gate has given up and
// the armed launches ran (or are running) on stale input -- the caller opens the word anyway, lets them drain and starts over.
static bool gate_claim(tamcmc_ctx *c)
{
    __atomic_store_n(c->h_gate + TM_GATE_FIRING, c->gate_seq, __ATOMIC_SEQ_CST);
    return __atomic_load_n(c->h_gate + TM_GATE_EXPIRED, __ATOMIC_SEQ_CST) == c->gate_seq;
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
    if (!c->h_gate) {
        TM_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->h_gate), 256, hipHostMallocMapped | hipHostMallocCoherent));
        TM_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&c->dv_gate), c->h_gate, 0));
        std::memset(c->h_gate, 0, 256);
        c->gate_seq = 1;               // (0 is what the expiry / firing words hold before the first batch)
        *c->h_gate = c->gate_seq;
    }
    const uint32_t target = c->gate_seq + 1;
    TM_HIP(ctx_settle(c));
    c->enq_seq++;
    int rc = tm_launch_gate(c->dv_gate, target, c->gate_patience, c->stream);
    if (rc != 0) { snprintf(g_hip_err, sizeof(g_hip_err), "gate launch -> %s", hipGetErrorString((hipError_t)rc)); return TAMCMC_E_HIP; }
    const size_t n = (size_t)Nchains;
    rc = enqueue(c, Nchains, c->dv_in, c->dv_in + n * c->L.Nparams, c->dv_out, nullptr, c->dv_status, nullptr, nullptr);
    c->gate_seq = target;
    if (rc != TAMCMC_OK) {            // the gate is in the stream: open it, nothing sits behind it
        __atomic_store_n(c->h_gate, target, __ATOMIC_RELEASE);
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
        __atomic_store_n(c->h_gate, c->gate_seq, __ATOMIC_RELEASE);
        c->armed = 0;
        TM_HIP(ctx_stream_sync(c));
        return tamcmc_eval_batch_begin(c, Nchains, Nparams, params, Tcoefs);
    }
    const size_t n = (size_t)Nchains;
    std::memcpy(c->h_in, params, n * Nparams * sizeof(double));
    std::memcpy(c->h_in + n * Nparams, Tcoefs, n * sizeof(double));
    mark_pending(c, Nchains, (size_t)Nchains);
    __atomic_store_n(c->h_gate, c->gate_seq, __ATOMIC_RELEASE);      // (after the parameters and the markers)
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
        __atomic_store_n(c->h_gate, c->gate_seq, __ATOMIC_RELEASE);
        c->armed = 0;
        TM_HIP(ctx_stream_sync(c));
        return TAMCMC_OK;
    }
    mark_pending(c, n, (size_t)n);
    __atomic_store_n(c->h_gate, c->gate_seq, __ATOMIC_RELEASE);
    c->ev_recorded = false;
    c->armed = 0;
    return wait_data(c, n, (size_t)n);
}

extern "C" int tamcmc_ctx_reserve(tamcmc_ctx *c, int32_t Nchains)
{
    if (!c || Nchains < 1 || c->in_flight || c->armed) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(c->device));
    int rc = ensure_capacity(c, Nchains, false);
    if (rc != TAMCMC_OK) return rc;
    return ensure_staging(c, Nchains);
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
    int rc = ensure_capacity(c, Nchains, grad != nullptr);
    if (rc != TAMCMC_OK) return rc;

    const size_t n = (size_t)Nchains;
    rc = ensure_staging(c, Nchains);
    if (rc != TAMCMC_OK) return rc;
    std::memcpy(c->h_in, params, n * Nparams * sizeof(double));
    std::memcpy(c->h_in + n * Nparams, Tcoefs, n * sizeof(double));
    double *dv_in = nullptr, *dv_out = nullptr;
    int32_t *dv_status = nullptr;
    dv_in = c->dv_in; dv_out = c->dv_out; dv_status = c->dv_status;
    const int32_t *d_rows = nullptr;
    if (n_rows > 0) {
        std::vector<int32_t> rows(n, -1);
        for (int r = 0; r < n_rows; r++) rows[(size_t)model_rows[r]] = r;   // a chain listed twice keeps the last row
        const size_t need = (size_t)n_rows * (size_t)c->L.Nx;
        if (need > c->model_cap) {
            TM_HIP(ctx_stream_sync(c));
            (void)hipFree(c->d_model); c->d_model = nullptr; c->model_cap = 0;
            TM_HIP(hipMalloc(&c->d_model, need * sizeof(double)));
            c->model_cap = need;
        }
        TM_HIP(hipMemcpyAsync(c->d_rows, rows.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        TM_HIP(ctx_stream_sync(c));   // rows is a local
        d_rows = c->d_rows;
    }
    // logL / status (a few hundred bytes) are written straight into the mapped host buffer by the last kernel; the
    // the backward kernel writes each chain's gradient row as one run of consecutive stores, straight into the mapped
    // host buffer (a copy-engine transfer of these ~20 KB would add ~20 us of latency)
    const bool watch = (n_rows == 0);                         // no model rows to copy back: watch the results arrive (wait_data)
    const size_t nwatch = n * (grad ? (size_t)c->Nvars + 1 : 1);
    if (watch) mark_pending(c, Nchains, nwatch);
    rc = enqueue(c, Nchains, dv_in, dv_in + n * Nparams, dv_out, grad ? dv_out + n : nullptr, dv_status, d_rows, c->d_model);
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
    std::memcpy(logL, c->h_out, n * sizeof(double));
    if (status) std::memcpy(status, c->h_status, n * sizeof(int32_t));
    if (grad) std::memcpy(grad, c->h_out + n, n * (size_t)c->Nvars * sizeof(double));
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

// ---------------------------------------------------------------------------------------------------------------------
// Fit groups (tamcmc_accel.h, tamcmc_group.h): the likelihood batches of several contexts in one launch per kernel kind.
struct tamcmc_group {
    int device = 0;
    std::vector<tamcmc_ctx *> m;
    hipStream_t own_stream = nullptr, stream = nullptr;
    std::vector<hipEvent_t> ev_before;   // per member: recorded on its stream, waited for by the group stream
    hipEvent_t ev_after = nullptr;       // recorded on the group stream after a call's launches, waited for by the members
    hipEvent_t ev_done = nullptr;        // completion of a host-pointer call (polled)
    // descriptor table: one device copy (rewritten in stream order) from two pinned host images, so that the image a
    // pending upload reads is never the one being filled
    // (one device copy per caller: 0 tamcmc_group_eval / _eval_device, 1 and 2 the two input buffers of _eval_begin --
    // a caller whose chain counts do not change finds its table in place and uploads nothing)
    struct Tab { char *d = nullptr; size_t cap = 0; std::vector<char> last; } tab[3];   // (last: the table as uploaded)
    char *h_tab[2] = {nullptr, nullptr};
    size_t h_tab_cap[2] = {0, 0};
    hipEvent_t ev_tab[2] = {nullptr, nullptr};
    bool tab_pending[2] = {false, false};
    int tab_slot = 0;
    // host-pointer calls: one pinned staging area [params | Tcoefs | logL | status] and its device copy
    char *h_stage = nullptr, *d_stage = nullptr;
    size_t stage_cap = 0;
    bool counted = false;                // the members' group counts include this group (set once creation succeeded)
    // _eval_begin / _end / _poll: mapped, coherent pinned staging [params | Tcoefs | logL | status] the grouped kernels
    // read and write directly, one per call parity (filling the inputs of call n+1 never touches what a kernel of call n
    // may still read)
    char *h_map[2] = {nullptr, nullptr}, *dv_map[2] = {nullptr, nullptr};
    size_t map_cap[2] = {0, 0};
    int parity = 0;
    int flight = 0;                      // chains of the batch in flight (0: none)
    std::vector<int32_t> fl_off;         // [members + 1] first slot of each member's block in the batch in flight
    uint64_t *fl_out = nullptr;          // its result slots (host view): logL, status
    int32_t *fl_st = nullptr;
    bool ev_recorded = false;            // wait_slots: ev_done has been recorded for the batch in flight
    std::vector<uint64_t> seen_seq;      // per member: its enq_seq when the group stream last ordered itself after its stream
    std::vector<hipStream_t> seen_stream;
};

static bool generic_body(const tamcmc_ctx *c) { return eval_args(c, 1, false, nullptr, nullptr, nullptr, nullptr).generic != 0; }

// Everything a group call refuses, checked before anything is allocated or enqueued.
static int group_check(const tamcmc_group *g, const int32_t *Nchains, const int32_t *Nparams)
{
    if (!g || !Nchains || !Nparams) return TAMCMC_E_INVALID;
    long long total = 0, wg_setup = 0, wg_fused = 0, wg_eval[2] = {0, 0};
    for (size_t k = 0; k < g->m.size(); k++) {
        const tamcmc_ctx *c = g->m[k];
        const int nc = Nchains[k];
        if (nc < 0 || Nparams[k] != c->L.Nparams || c->armed || c->in_flight) return TAMCMC_E_INVALID;
        if (nc == 0) continue;
        if (c->nspec > 1 && (c->d_spec == nullptr || nc > c->spec_n)) return TAMCMC_E_INVALID;   // the map must cover the batch
        total += nc;
        const int tiles = pick_tiles(c, nc, false);
        if (takes_fused(c, tiles)) wg_fused += nc;
        else { wg_setup += nc; wg_eval[generic_body(c) ? 1 : 0] += (long long)nc * tiles; }
    }
    if (total < 1) return TAMCMC_E_INVALID;
    // 1-D launches: workgroups x threads must stay within 32 bits
    const long long lim = 0xFFFFFFFFLL;
    if (wg_setup > lim / TM_SETUP_THREADS || wg_fused > lim / TM_THREADS || wg_eval[0] > lim / TM_THREADS ||
        wg_eval[1] > lim / TM_THREADS)
        return TAMCMC_E_INVALID;
    return TAMCMC_OK;
}

// Uploads the table when it differs from the one the device holds (stream-ordered: launches already enqueued keep
// reading the previous contents).
static int group_upload(tamcmc_group *g, const std::vector<char> &tab, int tslot)
{
    tamcmc_group::Tab &t = g->tab[tslot];
    if (tab == t.last) return TAMCMC_OK;
    if (tab.size() > t.cap) {
        TM_HIP(hipStreamSynchronize(g->stream));
        (void)hipFree(t.d); t.d = nullptr; t.cap = 0;
        TM_HIP(hipMalloc(&t.d, tab.size()));
        t.cap = tab.size();
    }
    const int s = g->tab_slot ^= 1;
    if (g->tab_pending[s]) { TM_HIP(hipEventSynchronize(g->ev_tab[s])); g->tab_pending[s] = false; }
    if (tab.size() > g->h_tab_cap[s]) {
        (void)hipHostFree(g->h_tab[s]); g->h_tab[s] = nullptr; g->h_tab_cap[s] = 0;
        TM_HIP(hipHostMalloc(reinterpret_cast<void **>(&g->h_tab[s]), tab.size(), hipHostMallocDefault));
        g->h_tab_cap[s] = tab.size();
    }
    std::memcpy(g->h_tab[s], tab.data(), tab.size());
    t.last.clear();                      // (a failed copy leaves no claim about the device contents)
    TM_HIP(hipMemcpyAsync(t.d, g->h_tab[s], tab.size(), hipMemcpyHostToDevice, g->stream));
    TM_HIP(hipEventRecord(g->ev_tab[s], g->stream));
    g->tab_pending[s] = true;
    t.last = tab;
    return TAMCMC_OK;
}

// Enqueue one group call on the group stream: member k's chains read Nchains[k] rows of Nparams[k] from d_params (blocks
// in member order) and write their logL / status at their offset in the concatenated outputs.  group_check has passed.
// tslot: the device table to use (tamcmc_group::tab).  lazy: the members' streams are not made to wait here; each gets
// the group's event to wait for before its next use (ctx_settle), and a member on whose own stream nothing was enqueued
// since the group last ordered itself after it is not waited for either.
static int group_enqueue(tamcmc_group *g, const int32_t *Nchains, const double *d_params, const double *d_T, double *d_logL,
                         int32_t *d_status, int tslot = 0, bool lazy = false)
{
    const int n = (int)g->m.size();
    bool grow = false;
    for (int k = 0; k < n; k++) grow = grow || Nchains[k] > g->m[k]->cap;
    if (grow) TM_HIP(hipStreamSynchronize(g->stream));   // an earlier group launch may still use the buffers about to move
    for (int k = 0; k < n; k++)
        if (Nchains[k] > 0) { const int rc = ensure_capacity(g->m[k], Nchains[k], false); if (rc != TAMCMC_OK) return rc; }

    std::vector<TmGroupSetup> su;
    std::vector<TmGroupFused> fu;
    std::vector<TmEvalArgs> ev[2];
    std::vector<int32_t> su_pre{0}, fu_pre{0}, ev_pre[2] = {{0}, {0}}, ev_nch[2];
    size_t lds_su = 8, lds_fu = 8;
    size_t po = 0, co = 0;
    for (int k = 0; k < n; k++) {
        tamcmc_ctx *c = g->m[k];
        const int nc = Nchains[k];
        if (nc > 0) {
            const int tiles = pick_tiles(c, nc, false);
            const double *P = d_params + po, *T = d_T + co;
            const TmEvalArgs a = eval_args(c, tiles, false, d_logL + co, d_status ? d_status + co : nullptr, nullptr, nullptr);
            const int p_doubles = (c->L.Nparams + 1) & ~1;
            if (takes_fused(c, tiles)) {
                TmGroupFused d{};
                d.L = c->L; d.a = a;
                d.f.params = P; d.f.Tcoefs = T; d.f.p_doubles = p_doubles;
                fu.push_back(d);
                fu_pre.push_back(fu_pre.back() + nc);
                lds_fu = std::max(lds_fu, ((size_t)p_doubles + 1) * sizeof(double));     // as tm_launch_fused
            } else {
                TmGroupSetup d{};
                d.L = c->L; d.params = P; d.Tcoefs = T; d.wt = c->d_wt; d.lx = c->d_lx;
                d.mult = c->d_mult; d.noise = c->d_noise; d.cell = c->d_cell; d.thdr = c->d_thdr; d.tidx = c->d_tidx;
                d.order = (a.order_mode == 2) ? c->d_order : nullptr;
                d.cm = c->cost_l; d.units = c->units; d.cells = c->cells; d.tiles = tiles;
                d.eq = tm_setup_balances(c->units, tiles, c->equal_cost, c->cost_l.pad);
                d.p_doubles = p_doubles;
                su.push_back(d);
                su_pre.push_back(su_pre.back() + nc);
                lds_su = std::max(lds_su, (size_t)p_doubles * sizeof(double) + (d.eq ? (size_t)c->units * sizeof(int) : 0));   // as tm_launch_setup
                const int gen = a.generic ? 1 : 0;
                ev[gen].push_back(a);
                ev_pre[gen].push_back(ev_pre[gen].back() + nc * tiles);
                ev_nch[gen].push_back(nc);
            }
        }
        po += (size_t)nc * (size_t)c->L.Nparams;
        co += (size_t)nc;
    }
    // the table, one section per array at 256-byte boundaries (tamcmc_group.h)
    std::vector<char> tab;
    auto put = [&](const void *src, size_t bytes) {
        const size_t off = (tab.size() + 255) & ~(size_t)255;
        tab.resize(off + (bytes > 0 ? bytes : 1));
        if (bytes) std::memcpy(tab.data() + off, src, bytes);
        return off;
    };
    const size_t o_su_pre = put(su_pre.data(), su_pre.size() * sizeof(int32_t)), o_su = put(su.data(), su.size() * sizeof(TmGroupSetup));
    const size_t o_fu_pre = put(fu_pre.data(), fu_pre.size() * sizeof(int32_t)), o_fu = put(fu.data(), fu.size() * sizeof(TmGroupFused));
    size_t o_ev_pre[2], o_ev_nch[2], o_ev[2];
    for (int gen = 0; gen < 2; gen++) {
        o_ev_pre[gen] = put(ev_pre[gen].data(), ev_pre[gen].size() * sizeof(int32_t));
        o_ev_nch[gen] = put(ev_nch[gen].data(), ev_nch[gen].size() * sizeof(int32_t));
        o_ev[gen] = put(ev[gen].data(), ev[gen].size() * sizeof(TmEvalArgs));
    }

    // work enqueued earlier on a member's stream comes first
    for (int k = 0; k < n; k++) {
        tamcmc_ctx *c = g->m[k];
        if (Nchains[k] > 0 && c->stream != g->stream) {
            // an event another group left for this stream goes onto it first (and counts as work enqueued there); this
            // group's own is on the group stream already
            if (c->after_ev && c->after_owner != g) { TM_HIP(ctx_settle(c)); c->enq_seq++; }
            // (a stream handed in by the caller may carry work this library has not counted)
            if (c->stream == c->own_stream && g->seen_stream[k] == c->stream && g->seen_seq[k] == c->enq_seq) continue;
            TM_HIP(hipEventRecord(g->ev_before[k], c->stream));
            TM_HIP(hipStreamWaitEvent(g->stream, g->ev_before[k], 0));
            g->seen_stream[k] = c->stream; g->seen_seq[k] = c->enq_seq;
        }
    }
    int rc = group_upload(g, tab, tslot);
    if (rc != TAMCMC_OK) return rc;
    const char *D = g->tab[tslot].d;
    const char *what = "";
    int hr = 0;
    if (!su.empty()) {
        what = "group setup launch";
        hr = tm_launch_group_setup(reinterpret_cast<const TmGroupSetup *>(D + o_su), reinterpret_cast<const int32_t *>(D + o_su_pre),
                                   (int)su.size(), su_pre.back(), lds_su, g->stream);
    }
    if (hr == 0 && !fu.empty()) {
        what = "group fused launch";
        hr = tm_launch_group_fused(reinterpret_cast<const TmGroupFused *>(D + o_fu), reinterpret_cast<const int32_t *>(D + o_fu_pre),
                                   (int)fu.size(), fu_pre.back(), lds_fu, g->stream);
    }
    for (int gen = 0; gen < 2 && hr == 0; gen++) {
        if (ev[gen].empty()) continue;
        what = "group eval launch";
        hr = tm_launch_group_eval(reinterpret_cast<const TmEvalArgs *>(D + o_ev[gen]), reinterpret_cast<const int32_t *>(D + o_ev_pre[gen]),
                                  reinterpret_cast<const int32_t *>(D + o_ev_nch[gen]), (int)ev[gen].size(), ev_pre[gen].back(),
                                  gen == 1, g->stream);
    }
    if (hr != 0) {
        snprintf(g_hip_err, sizeof(g_hip_err), "%s -> %s", what, hipGetErrorString((hipError_t)hr));
        for (int k = 0; k < n; k++)        // arrival counters back to zero
            if (Nchains[k] > 0) (void)hipMemsetAsync(g->m[k]->d_ticket, 0, (size_t)Nchains[k] * sizeof(int32_t), g->stream);
        rc = TAMCMC_E_HIP;
    }
    // and later work on a member's stream comes after
    if (hipEventRecord(g->ev_after, g->stream) != hipSuccess) return TAMCMC_E_HIP;
    for (int k = 0; k < n; k++) {
        tamcmc_ctx *c = g->m[k];
        if (Nchains[k] == 0 || c->stream == g->stream) continue;
        if (lazy) { c->after_ev = g->ev_after; c->after_owner = g; continue; }
        if (c->after_owner == g) { c->after_ev = nullptr; c->after_owner = nullptr; }     // (the wait below covers it)
        if (hipStreamWaitEvent(c->stream, g->ev_after, 0) != hipSuccess) return TAMCMC_E_HIP;
        c->enq_seq++;
    }
    return rc;
}

// The batch in flight of tamcmc_group_eval_begin: wait until every result slot holds its final value (wait_slots: a
// failed launch ends the wait with an error and the members' arrival counters are put back to zero).
static int group_drain(tamcmc_group *g)
{
    const int n = g->flight;
    const TmWatch w{g->fl_out, g->fl_st, &g->ev_done, &g->ev_recorded, g->stream};
    const int rc = wait_slots(w, n, (size_t)n, [g]() {
        for (size_t k = 0; k < g->m.size(); k++) {
            const int nc = g->fl_off[k + 1] - g->fl_off[k];
            if (nc > 0) (void)hipMemsetAsync(g->m[k]->d_ticket, 0, (size_t)nc * sizeof(int32_t), g->stream);
        }
    });
    g->flight = 0;                   // (only now: _poll is answered until the batch is closed)
    return rc;
}

extern "C" int tamcmc_group_create(tamcmc_group **out, int32_t n_members, tamcmc_ctx *const *members)
{
    if (!out) return TAMCMC_E_INVALID;
    *out = nullptr;
    if (n_members < 1 || n_members > TM_GROUP_MAX_MEMBERS || !members) return TAMCMC_E_INVALID;
    for (int k = 0; k < n_members; k++) {
        if (!members[k] || members[k]->device != members[0]->device) return TAMCMC_E_INVALID;
        for (int j = 0; j < k; j++) if (members[j] == members[k]) return TAMCMC_E_INVALID;
    }
    tamcmc_group *g = new (std::nothrow) tamcmc_group();
    if (!g) return TAMCMC_E_NOMEM;
    g->device = members[0]->device;
    g->m.assign(members, members + n_members);
    g->ev_before.assign((size_t)n_members, nullptr);
    g->seen_seq.assign((size_t)n_members, ~(uint64_t)0);
    g->seen_stream.assign((size_t)n_members, nullptr);
    auto fail = [&](int code) { tamcmc_group_destroy(g); return code; };
    if (hipSetDevice(g->device) != hipSuccess) return fail(TAMCMC_E_NODEVICE);
    if (hipStreamCreateWithFlags(&g->own_stream, hipStreamNonBlocking) != hipSuccess) return fail(TAMCMC_E_HIP);
    g->stream = g->own_stream;
    for (auto &e : g->ev_before) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return fail(TAMCMC_E_HIP);
    if (hipEventCreateWithFlags(&g->ev_after, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&g->ev_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&g->ev_tab[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&g->ev_tab[1], hipEventDisableTiming) != hipSuccess)
        return fail(TAMCMC_E_HIP);
    for (tamcmc_ctx *c : g->m) c->groups++;
    g->counted = true;
    *out = g;
    return TAMCMC_OK;
}

extern "C" int tamcmc_group_destroy(tamcmc_group *g)
{
    if (!g) return TAMCMC_OK;
    (void)hipSetDevice(g->device);
    if (g->flight) (void)group_drain(g);           // a batch in flight: wait for it, hand nothing out
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    for (tamcmc_ctx *c : g->m)                     // (everything of this group has retired: nothing left to wait for)
        if (c->after_owner == g) { c->after_ev = nullptr; c->after_owner = nullptr; }
    if (g->counted) for (tamcmc_ctx *c : g->m) c->groups--;
    for (auto &t : g->tab) (void)hipFree(t.d);
    (void)hipFree(g->d_stage);
    (void)hipHostFree(g->h_map[0]); (void)hipHostFree(g->h_map[1]);
    (void)hipHostFree(g->h_tab[0]); (void)hipHostFree(g->h_tab[1]); (void)hipHostFree(g->h_stage);
    for (hipEvent_t e : g->ev_before) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {g->ev_after, g->ev_done, g->ev_tab[0], g->ev_tab[1]}) if (e) (void)hipEventDestroy(e);
    if (g->own_stream) (void)hipStreamDestroy(g->own_stream);
    delete g;
    return TAMCMC_OK;
}

extern "C" int tamcmc_group_set_stream(tamcmc_group *g, void *hip_stream)
{
    if (!g || g->flight) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(g->device));
    TM_HIP(hipStreamSynchronize(g->stream));
    g->stream = hip_stream ? (hipStream_t)hip_stream : g->own_stream;
    return TAMCMC_OK;
}

extern "C" int tamcmc_group_synchronize(tamcmc_group *g)
{
    if (!g || g->flight) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(g->device));
    TM_HIP(hipStreamSynchronize(g->stream));
    return TAMCMC_OK;
}

extern "C" int tamcmc_group_eval_device(tamcmc_group *g, const int32_t *Nchains, const int32_t *Nparams, const double *d_params,
                                        const double *d_Tcoefs, double *d_logL, int32_t *d_status)
{
    if (g && g->flight) return TAMCMC_E_INVALID;      // a batch of _eval_begin is in flight: _eval_end first
    int rc = group_check(g, Nchains, Nparams);
    if (rc != TAMCMC_OK) return rc;
    if (!d_params || !d_Tcoefs || !d_logL) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(g->device));
    return group_enqueue(g, Nchains, d_params, d_Tcoefs, d_logL, d_status);
}

extern "C" int tamcmc_group_eval(tamcmc_group *g, const int32_t *Nchains, const int32_t *Nparams, const double *params,
                                 const double *Tcoefs, double *logL, int32_t *status)
{
    if (g && g->flight) return TAMCMC_E_INVALID;      // a batch of _eval_begin is in flight: _eval_end first
    int rc = group_check(g, Nchains, Nparams);
    if (rc != TAMCMC_OK) return rc;
    if (!params || !Tcoefs || !logL) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(g->device));
    size_t np = 0, nc = 0;
    for (size_t k = 0; k < g->m.size(); k++) { np += (size_t)Nchains[k] * (size_t)Nparams[k]; nc += (size_t)Nchains[k]; }
    // staging [params | Tcoefs | logL | status]: one copy in, one copy out
    const size_t o_out = (np + nc) * sizeof(double), bytes_out = nc * (sizeof(double) + sizeof(int32_t)), bytes = o_out + bytes_out;
    if (bytes > g->stage_cap) {
        TM_HIP(hipStreamSynchronize(g->stream));
        (void)hipHostFree(g->h_stage); (void)hipFree(g->d_stage);
        g->h_stage = g->d_stage = nullptr; g->stage_cap = 0;
        TM_HIP(hipHostMalloc(reinterpret_cast<void **>(&g->h_stage), bytes, hipHostMallocDefault));
        TM_HIP(hipMalloc(&g->d_stage, bytes));
        g->stage_cap = bytes;
    }
    std::memcpy(g->h_stage, params, np * sizeof(double));
    std::memcpy(g->h_stage + np * sizeof(double), Tcoefs, nc * sizeof(double));
    // from here on, a failure waits for the stream before it returns: a copy from or into h_stage may still be pending,
    // and the next call refills it
    auto fail = [&](int code) { (void)hipStreamSynchronize(g->stream); return code; };
    hipError_t e = hipMemcpyAsync(g->d_stage, g->h_stage, o_out, hipMemcpyHostToDevice, g->stream);
    if (e != hipSuccess) { snprintf(g_hip_err, sizeof(g_hip_err), "group input copy -> %s", hipGetErrorString(e)); return fail(TAMCMC_E_HIP); }
    double *d_in = reinterpret_cast<double *>(g->d_stage);
    double *d_logL = reinterpret_cast<double *>(g->d_stage + o_out);
    int32_t *d_status = reinterpret_cast<int32_t *>(g->d_stage + o_out + nc * sizeof(double));
    rc = group_enqueue(g, Nchains, d_in, d_in + np, d_logL, d_status);
    if (rc != TAMCMC_OK) return fail(rc);
    e = hipMemcpyAsync(g->h_stage + o_out, g->d_stage + o_out, bytes_out, hipMemcpyDeviceToHost, g->stream);
    if (e == hipSuccess) e = hipEventRecord(g->ev_done, g->stream);
    if (e != hipSuccess) { snprintf(g_hip_err, sizeof(g_hip_err), "group output copy -> %s", hipGetErrorString(e)); return fail(TAMCMC_E_HIP); }
    // wait by polling an event (see wait_done)
    for (;;) {
        e = hipEventQuery(g->ev_done);
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) { snprintf(g_hip_err, sizeof(g_hip_err), "hipEventQuery -> %s", hipGetErrorString(e)); return fail(TAMCMC_E_HIP); }
        __builtin_ia32_pause();
    }
    std::memcpy(logL, g->h_stage + o_out, nc * sizeof(double));
    if (status) std::memcpy(status, g->h_stage + o_out + nc * sizeof(double), nc * sizeof(int32_t));
    return TAMCMC_OK;
}

// The host-pointer call in two halves, on mapped memory: no copy-engine transfer and no event on the way of a healthy call.
extern "C" int tamcmc_group_eval_begin(tamcmc_group *g, const int32_t *Nchains, const int32_t *Nparams, const double *params,
                                       const double *Tcoefs)
{
    if (g && g->flight) return TAMCMC_E_INVALID;      // one batch in flight per group
    int rc = group_check(g, Nchains, Nparams);
    if (rc != TAMCMC_OK) return rc;
    if (!params || !Tcoefs) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(g->device));
    const size_t nm = g->m.size();
    size_t np = 0, nc = 0;
    g->fl_off.assign(nm + 1, 0);
    for (size_t k = 0; k < nm; k++) {
        np += (size_t)Nchains[k] * (size_t)Nparams[k]; nc += (size_t)Nchains[k];
        g->fl_off[k + 1] = (int32_t)nc;
    }
    if (nc > 0x7FFFFFFFu) return TAMCMC_E_INVALID;
    const int p = g->parity ^= 1;
    const size_t o_out = (np + nc) * sizeof(double), bytes = o_out + nc * (sizeof(double) + sizeof(int32_t));
    if (bytes > g->map_cap[p]) {
        TM_HIP(hipStreamSynchronize(g->stream));       // (a launch of two calls ago may not have retired yet)
        (void)hipHostFree(g->h_map[p]); g->h_map[p] = g->dv_map[p] = nullptr; g->map_cap[p] = 0;
        const size_t cap = bytes + bytes / 2;
        TM_HIP(hipHostMalloc(reinterpret_cast<void **>(&g->h_map[p]), cap, hipHostMallocMapped | hipHostMallocCoherent));
        TM_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&g->dv_map[p]), g->h_map[p], 0));
        g->map_cap[p] = cap;
    }
    char *h = g->h_map[p], *dv = g->dv_map[p];
    std::memcpy(h, params, np * sizeof(double));
    std::memcpy(h + np * sizeof(double), Tcoefs, nc * sizeof(double));
    g->fl_out = reinterpret_cast<uint64_t *>(h + o_out);
    g->fl_st = reinterpret_cast<int32_t *>(h + o_out + nc * sizeof(double));
    const TmWatch w{g->fl_out, g->fl_st, &g->ev_done, &g->ev_recorded, g->stream};
    mark_slots(w, (int)nc, nc);
    double *d_in = reinterpret_cast<double *>(dv);
    rc = group_enqueue(g, Nchains, d_in, d_in + np, reinterpret_cast<double *>(dv + o_out),
                       reinterpret_cast<int32_t *>(dv + o_out + nc * sizeof(double)), 1 + p, true);
    if (rc != TAMCMC_OK) {
        // whatever did get launched may still write into this buffer: let it retire before the buffer is reused
        (void)hipStreamSynchronize(g->stream);
        return rc;
    }
    g->ev_recorded = false;          // wait_slots records the completion event only if the results are slow to arrive
    g->flight = (int)nc;
    return TAMCMC_OK;
}

extern "C" int tamcmc_group_eval_end(tamcmc_group *g, double *logL, int32_t *status)
{
    if (!g || !logL || !g->flight) return TAMCMC_E_INVALID;
    const size_t nc = (size_t)g->flight;
    TM_HIP(hipSetDevice(g->device));
    const int rc = group_drain(g);
    if (rc != TAMCMC_OK) return rc;
    std::memcpy(logL, g->fl_out, nc * sizeof(double));
    if (status) std::memcpy(status, g->fl_st, nc * sizeof(int32_t));
    return TAMCMC_OK;
}

extern "C" int tamcmc_group_eval_poll(const tamcmc_group *g, int32_t member, int32_t chain, double *logL, int32_t *status)
{
    if (!g || !logL || !status || !g->flight || member < 0 || (size_t)member >= g->m.size() || chain < 0) return TAMCMC_E_INVALID;
    const int32_t o = g->fl_off[(size_t)member];
    if (chain >= g->fl_off[(size_t)member + 1] - o) return TAMCMC_E_INVALID;
    return poll_slot(g->fl_out, g->fl_st, (size_t)(o + chain), logL, status);
}

extern "C" int tamcmc_group_members(const tamcmc_group *g, int32_t *n_members, int32_t *Nparams, int32_t *device)
{
    if (!g) return TAMCMC_E_INVALID;
    if (n_members) *n_members = (int32_t)g->m.size();
    if (Nparams) for (size_t k = 0; k < g->m.size(); k++) Nparams[k] = g->m[k]->L.Nparams;
    if (device) *device = g->device;
    return TAMCMC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Posterior summaries of a stored chain (tamcmc_accel.h, tamcmc_summary.h): per-bin running statistics of the model and
// of the pointwise log-likelihood over the samples pushed so far.  A block of samples = the context's own launches with
// a row map covering every chain (stage 1) + tamcmc_summary_fold_kernel (stage 2), both on the context's stream.
struct tamcmc_summary {
    tamcmc_ctx *c = nullptr;
    int B = 0;                           // samples per block
    bool counted = false;                // the context's count includes this object
    double *d_model = nullptr;           // [B][Nx] model rows of the block in flight (the context's d_model is not touched)
    double *d_state = nullptr;           // [TM_SUM_NSTATE][Nx]
    long long *d_cnt = nullptr;          // [2][2] {accepted, rejected}: launch k reads pair k & 1 and writes the other
    int parity = 0;
    int32_t *d_rows = nullptr;           // [B] the identity row map
    double *d_T = nullptr;               // [B] ones: samples are evaluated at temperature 1
    double *d_logL = nullptr;            // [B] / [B]: where a block's logL / status go when the caller wants none
    int32_t *d_status = nullptr;
    // host-pointer pushes: [params | logL | status] of a block, pinned and on the device, two of each (block k fills
    // slot k & 1 while block k - 1 may still be read by its copies)
    char *h_stage[2] = {nullptr, nullptr}, *d_stage[2] = {nullptr, nullptr};
    hipEvent_t ev_stage[2] = {nullptr, nullptr};
    // timing of the fold kernel alone (tamcmc_summary_profile)
    bool profile = false;
    std::vector<hipEvent_t> ev;
    size_t ev_used = 0;
};

static size_t summary_stage_out(const tamcmc_summary *s) { return (size_t)s->B * (size_t)s->c->L.Nparams * sizeof(double); }
static size_t summary_stage_bytes(const tamcmc_summary *s) { return summary_stage_out(s) + (size_t)s->B * (sizeof(double) + sizeof(int32_t)); }

// what every push refuses (the context's state may have changed since the object was created)
static int summary_check(const tamcmc_summary *s, int32_t Nsamples, int32_t Nparams, const double *params)
{
    if (!s || !params || Nsamples < 1) return TAMCMC_E_INVALID;
    const tamcmc_ctx *c = s->c;
    if (Nparams != c->L.Nparams || c->in_flight || c->armed || c->nspec > 1) return TAMCMC_E_INVALID;
    return TAMCMC_OK;
}

// One block of n <= B samples, device pointers, enqueued on the context's stream.
static int summary_block(tamcmc_summary *s, int n, const double *d_params, double *d_logL, int32_t *d_status)
{
    tamcmc_ctx *c = s->c;
    int rc = ensure_capacity(c, n, false);
    if (rc != TAMCMC_OK) return rc;
    if (!d_logL) d_logL = s->d_logL;
    if (!d_status) d_status = s->d_status;
    rc = enqueue(c, n, d_params, s->d_T, d_logL, nullptr, d_status, s->d_rows, s->d_model);
    if (rc != TAMCMC_OK) return rc;
    TmSummaryArgs a{};
    a.rows = s->d_model; a.status = d_status; a.y = c->d_y; a.isig2 = c->d_isig2; a.state = s->d_state;
    a.cnt_in = s->d_cnt + 2 * s->parity; a.cnt_out = s->d_cnt + 2 * (s->parity ^ 1);
    a.Nx = c->L.Nx; a.B = n; a.likelihood_case = c->L.likelihood_case; a.like_p = c->L.like_p;
    if (s->profile) {
        while (s->ev.size() < s->ev_used + 2) {
            hipEvent_t e;
            TM_HIP(hipEventCreate(&e));
            s->ev.push_back(e);
        }
        TM_HIP(hipEventRecord(s->ev[s->ev_used], c->stream));
    }
    const int hr = tm_launch_summary_fold(a, c->stream);
    if (hr != 0) { snprintf(g_hip_err, sizeof(g_hip_err), "summary fold launch -> %s", hipGetErrorString((hipError_t)hr)); return TAMCMC_E_HIP; }
    s->parity ^= 1;
    if (s->profile) {
        TM_HIP(hipEventRecord(s->ev[s->ev_used + 1], c->stream));
        s->ev_used += 2;
    }
    return TAMCMC_OK;
}

static int summary_clear(tamcmc_summary *s)
{
    const tamcmc_ctx *c = s->c;
    TM_HIP(hipMemsetAsync(s->d_state, 0, (size_t)TM_SUM_NSTATE * (size_t)c->L.Nx * sizeof(double), c->stream));
    TM_HIP(hipMemsetAsync(s->d_cnt, 0, 4 * sizeof(long long), c->stream));
    s->parity = 0;
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_create(tamcmc_summary **out, tamcmc_ctx *c, int32_t block_chains)
{
    if (!out) return TAMCMC_E_INVALID;
    *out = nullptr;
    if (!c || block_chains < 0 || c->in_flight || c->armed) return TAMCMC_E_INVALID;
    if (c->nspec > 1) return TAMCMC_E_INVALID;      // several spectra in one context: out of scope
    tamcmc_summary *s = new (std::nothrow) tamcmc_summary();
    if (!s) return TAMCMC_E_NOMEM;
    s->c = c;
    const size_t nx = (size_t)c->L.Nx;
    int B = block_chains;
    if (B == 0) {                                   // 64, lowered so that a block's rows take at most 64 MiB
        const size_t fit = ((size_t)64 << 20) / (nx * sizeof(double));
        B = fit >= 64 ? 64 : (fit >= 1 ? (int)fit : 1);
    }
    s->B = B;
    auto fail = [&](int code) { tamcmc_summary_destroy(s); return code; };
    if (hipSetDevice(c->device) != hipSuccess) return fail(TAMCMC_E_NODEVICE);
    const size_t b = (size_t)B;
    if (hipMalloc(&s->d_model, b * nx * sizeof(double)) != hipSuccess || hipMalloc(&s->d_state, TM_SUM_NSTATE * nx * sizeof(double)) != hipSuccess ||
        hipMalloc(&s->d_cnt, 4 * sizeof(long long)) != hipSuccess || hipMalloc(&s->d_rows, b * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&s->d_T, b * sizeof(double)) != hipSuccess || hipMalloc(&s->d_logL, b * sizeof(double)) != hipSuccess ||
        hipMalloc(&s->d_status, b * sizeof(int32_t)) != hipSuccess)
        return fail(TAMCMC_E_NOMEM);
    {
        std::vector<int32_t> rows(b);
        std::vector<double> ones(b, 1.0);
        for (size_t k = 0; k < b; k++) rows[k] = (int32_t)k;
        if (hipMemcpy(s->d_rows, rows.data(), b * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(s->d_T, ones.data(), b * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
            return fail(TAMCMC_E_HIP);
    }
    if (ctx_settle(c) != hipSuccess || summary_clear(s) != TAMCMC_OK) return fail(TAMCMC_E_HIP);
    c->enq_seq++;
    c->summaries++;
    s->counted = true;
    *out = s;
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_destroy(tamcmc_summary *s)
{
    if (!s) return TAMCMC_OK;
    tamcmc_ctx *c = s->c;
    if (c->armed) return TAMCMC_E_INVALID;          // the stream cannot be waited for behind a closed gate: _fire or _disarm first
    (void)hipSetDevice(c->device);
    if (c->stream) (void)ctx_stream_sync(c);
    if (s->counted) c->summaries--;
    (void)hipFree(s->d_model); (void)hipFree(s->d_state); (void)hipFree(s->d_cnt); (void)hipFree(s->d_rows);
    (void)hipFree(s->d_T); (void)hipFree(s->d_logL); (void)hipFree(s->d_status);
    for (int p = 0; p < 2; p++) {
        (void)hipHostFree(s->h_stage[p]); (void)hipFree(s->d_stage[p]);
        if (s->ev_stage[p]) (void)hipEventDestroy(s->ev_stage[p]);
    }
    for (hipEvent_t e : s->ev) (void)hipEventDestroy(e);
    delete s;
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_reset(tamcmc_summary *s)
{
    if (!s || s->c->in_flight || s->c->armed) return TAMCMC_E_INVALID;
    tamcmc_ctx *c = s->c;
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(ctx_settle(c));
    c->enq_seq++;
    return summary_clear(s);
}

extern "C" int tamcmc_summary_push_device(tamcmc_summary *s, int32_t Nsamples, int32_t Nparams, const double *d_params,
                                          double *d_logL, int32_t *d_status)
{
    int rc = summary_check(s, Nsamples, Nparams, d_params);
    if (rc != TAMCMC_OK) return rc;
    TM_HIP(hipSetDevice(s->c->device));
    for (int32_t k = 0; k < Nsamples; k += s->B) {
        const int n = Nsamples - k < s->B ? Nsamples - k : s->B;
        rc = summary_block(s, n, d_params + (size_t)k * (size_t)Nparams, d_logL ? d_logL + k : nullptr, d_status ? d_status + k : nullptr);
        if (rc != TAMCMC_OK) return rc;
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_push(tamcmc_summary *s, int32_t Nsamples, int32_t Nparams, const double *params,
                                   double *logL, int32_t *status)
{
    int rc = summary_check(s, Nsamples, Nparams, params);
    if (rc != TAMCMC_OK) return rc;
    tamcmc_ctx *c = s->c;
    TM_HIP(hipSetDevice(c->device));
    const size_t o_out = summary_stage_out(s), bytes = summary_stage_bytes(s), np = (size_t)Nparams;
    for (int p = 0; p < 2; p++) {
        if (s->h_stage[p]) continue;
        TM_HIP(hipHostMalloc(reinterpret_cast<void **>(&s->h_stage[p]), bytes, hipHostMallocDefault));
        TM_HIP(hipMalloc(&s->d_stage[p], bytes));
        TM_HIP(hipEventCreateWithFlags(&s->ev_stage[p], hipEventDisableTiming));
    }
    // slot p's copies have landed: hand its block's logL / status out (polled, see wait_done)
    int pend_k[2] = {-1, -1}, pend_n[2] = {0, 0};
    auto collect = [&](int p) -> int {
        if (pend_k[p] < 0) return TAMCMC_OK;
        for (;;) {
            const hipError_t e = hipEventQuery(s->ev_stage[p]);
            if (e == hipSuccess) break;
            if (e != hipErrorNotReady) { snprintf(g_hip_err, sizeof(g_hip_err), "hipEventQuery -> %s", hipGetErrorString(e)); return TAMCMC_E_HIP; }
            __builtin_ia32_pause();
        }
        const size_t n = (size_t)pend_n[p];
        if (logL) std::memcpy(logL + pend_k[p], s->h_stage[p] + o_out, n * sizeof(double));
        if (status) std::memcpy(status + pend_k[p], s->h_stage[p] + o_out + (size_t)s->B * sizeof(double), n * sizeof(int32_t));
        pend_k[p] = -1;
        return TAMCMC_OK;
    };
    // a failure waits for the stream before it returns: a copy from or into the pinned slots may still be pending
    auto fail = [&](int code) { (void)hipStreamSynchronize(c->stream); return code; };
    int slot = 0;
    for (int32_t k = 0; k < Nsamples; k += s->B, slot ^= 1) {
        const int n = Nsamples - k < s->B ? Nsamples - k : s->B;
        rc = collect(slot);
        if (rc != TAMCMC_OK) return fail(rc);
        std::memcpy(s->h_stage[slot], params + (size_t)k * np, (size_t)n * np * sizeof(double));
        char *d = s->d_stage[slot];
        if (ctx_settle(c) != hipSuccess ||
            hipMemcpyAsync(d, s->h_stage[slot], (size_t)n * np * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess)
            return fail(TAMCMC_E_HIP);
        rc = summary_block(s, n, reinterpret_cast<const double *>(d), reinterpret_cast<double *>(d + o_out),
                           reinterpret_cast<int32_t *>(d + o_out + (size_t)s->B * sizeof(double)));
        if (rc != TAMCMC_OK) return fail(rc);
        if (hipMemcpyAsync(s->h_stage[slot] + o_out, d + o_out, bytes - o_out, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipEventRecord(s->ev_stage[slot], c->stream) != hipSuccess)
            return fail(TAMCMC_E_HIP);
        pend_k[slot] = k; pend_n[slot] = n;
    }
    // the older of the two pending blocks first: the stream runs them in order
    rc = collect(slot);
    if (rc == TAMCMC_OK) rc = collect(slot ^ 1);
    if (rc != TAMCMC_OK) return fail(rc);
    TM_HIP(hipGetLastError());
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_result(tamcmc_summary *s, tamcmc_summary_totals *totals,
                                     double *mean_M, double *var_M, double *min_M, double *max_M,
                                     double *mean_l, double *var_l, double *lppd)
{
    if (!s || s->c->in_flight || s->c->armed) return TAMCMC_E_INVALID;
    tamcmc_ctx *c = s->c;
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(ctx_stream_sync(c));
    const size_t nx = (size_t)c->L.Nx;
    long long cnt[2] = {0, 0};
    std::vector<double> st;
    try { st.resize(TM_SUM_NSTATE * nx); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    TM_HIP(hipMemcpy(cnt, s->d_cnt + 2 * s->parity, sizeof(cnt), hipMemcpyDeviceToHost));
    TM_HIP(hipMemcpy(st.data(), s->d_state, st.size() * sizeof(double), hipMemcpyDeviceToHost));
    const long long n = cnt[0];
    const double nan = std::nan(""), dn = (double)n;
    long double lppd_total = 0.0L, p_waic = 0.0L;
    for (size_t i = 0; i < nx; i++) {
        const double vM = n >= 2 ? st[TM_SUM_M2_M * nx + i] / (dn - 1.0) : nan;
        const double vl = n >= 2 ? st[TM_SUM_M2_L * nx + i] / (dn - 1.0) : nan;
        const double lp = n >= 1 ? st[TM_SUM_LSE_A * nx + i] + std::log(st[TM_SUM_LSE_R * nx + i] / dn) : nan;
        if (mean_M) mean_M[i] = n >= 1 ? st[TM_SUM_MEAN_M * nx + i] : nan;
        if (var_M) var_M[i] = vM;
        if (min_M) min_M[i] = n >= 1 ? st[TM_SUM_MIN_M * nx + i] : nan;
        if (max_M) max_M[i] = n >= 1 ? st[TM_SUM_MAX_M * nx + i] : nan;
        if (mean_l) mean_l[i] = n >= 1 ? st[TM_SUM_MEAN_L * nx + i] : nan;
        if (var_l) var_l[i] = vl;
        if (lppd) lppd[i] = lp;
        lppd_total += (long double)lp;          // in bin order
        p_waic += (long double)vl;
    }
    if (totals) {
        totals->n_used = n;
        totals->n_rejected = cnt[1];
        totals->lppd_total = (double)lppd_total;
        totals->p_waic = (double)p_waic;
        totals->waic = (double)(-2.0L * (lppd_total - p_waic));
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_profile(tamcmc_summary *s, int enable)
{
    if (!s || s->c->armed) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(s->c->device));
    TM_HIP(ctx_stream_sync(s->c));
    s->profile = enable != 0;
    s->ev_used = 0;
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_kernel_time(tamcmc_summary *s, double *total_ms, int64_t *launches)
{
    if (!s || !total_ms || !launches || s->c->armed) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(s->c->device));
    TM_HIP(ctx_stream_sync(s->c));
    double t = 0.0;
    for (size_t i = 0; i + 1 < s->ev_used; i += 2) {
        float ms = 0.f;
        TM_HIP(hipEventElapsedTime(&ms, s->ev[i], s->ev[i + 1]));
        t += (double)ms;
    }
    *total_ms = t;
    *launches = (int64_t)(s->ev_used / 2);
    return TAMCMC_OK;
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

extern "C" const char *tamcmc_last_hip_error(void) { return g_hip_err; }
#ifndef TM_KERNEL_HASH
#define TM_KERNEL_HASH "unknown"
#endif
extern "C" const char *tamcmc_version(void) { return "tamcmc_accel 0.3 (gfx950) kernels:" TM_KERNEL_HASH; }
