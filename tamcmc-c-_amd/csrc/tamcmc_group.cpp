// tamcmc_group.cpp -- fit groups (tamcmc_accel.h, tamcmc_group.h): the likelihood batches of several contexts in one
// launch per kernel kind.  The members' buffers, launch arguments and stream ordering come from tamcmc_host.h.
#include <algorithm>
#include <new>

#include "tamcmc_host.h"
#include "tamcmc_group.h"

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
    TmPinned h_tab[2];
    hipEvent_t ev_tab[2] = {nullptr, nullptr};
    bool tab_pending[2] = {false, false};
    int tab_slot = 0;
    TmPinned stage;                      // host-pointer calls: one pinned staging area [params | Tcoefs | logL | status] and its device copy
    bool counted = false;                // the members' group counts include this group (set once creation succeeded)
    // _eval_begin / _end / _poll: mapped, coherent pinned staging [params | Tcoefs | logL | status] the grouped kernels
    // read and write directly, one per call parity (filling the inputs of call n+1 never touches what a kernel of call n
    // may still read)
    TmPinned map[2];
    int parity = 0;
    int flight = 0;                      // chains of the batch in flight (0: none)
    std::vector<int32_t> fl_off;         // [members + 1] first slot of each member's block in the batch in flight
    uint64_t *fl_out = nullptr;          // its result slots (host view): logL, status
    int32_t *fl_st = nullptr;
    bool ev_recorded = false;            // wait_slots: ev_done has been recorded for the batch in flight
    std::vector<uint64_t> seen_seq;      // per member: its enq_seq when the group stream last ordered itself after its stream
    std::vector<hipStream_t> seen_stream;
};

static bool generic_body(const tamcmc_ctx *c) { return tm_eval_args(c, 1, false, nullptr, nullptr, nullptr, nullptr).generic != 0; }

// Everything a group call refuses, checked before anything is allocated or enqueued.
static int group_check(const tamcmc_group *g, const int32_t *Nchains, const int32_t *Nparams)
{
    if (!g || g->flight || !Nchains || !Nparams) return TAMCMC_E_INVALID;     // (in flight: a batch of _eval_begin, _eval_end first)
    long long total = 0, wg_setup = 0, wg_fused = 0, wg_eval[2] = {0, 0};
    for (size_t k = 0; k < g->m.size(); k++) {
        const tamcmc_ctx *c = g->m[k];
        const int nc = Nchains[k];
        if (nc < 0 || Nparams[k] != c->L.Nparams || c->armed || c->in_flight) return TAMCMC_E_INVALID;
        if (nc == 0) continue;
        if (c->nspec > 1 && (c->d_spec == nullptr || nc > c->spec_n)) return TAMCMC_E_INVALID;   // the map must cover the batch
        total += nc;
        const int tiles = tm_ctx_tiles(c, false);
        if (tm_takes_fused(c, tiles)) wg_fused += nc;
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
    { const int rc = g->h_tab[s].reserve(tab.size(), TM_PIN_HOST); if (rc != TAMCMC_OK) return rc; }
    std::memcpy(g->h_tab[s].h, tab.data(), tab.size());
    t.last.clear();                      // (a failed copy leaves no claim about the device contents)
    TM_HIP(hipMemcpyAsync(t.d, g->h_tab[s].h, tab.size(), hipMemcpyHostToDevice, g->stream));
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
        if (Nchains[k] > 0) { const int rc = tm_ensure_capacity(g->m[k], Nchains[k], false); if (rc != TAMCMC_OK) return rc; }

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
            const int tiles = tm_ctx_tiles(c, false);
            const double *P = d_params + po, *T = d_T + co;
            const TmEvalArgs a = tm_eval_args(c, tiles, false, d_logL + co, d_status ? d_status + co : nullptr, nullptr, nullptr);
            const int p_doubles = (c->L.Nparams + 1) & ~1;
            if (tm_takes_fused(c, tiles)) {
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
            if (c->after_ev && c->after_owner != g) { TM_HIP(tm_ctx_settle(c)); c->enq_seq++; }
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
        what = "group setup";
        hr = tm_launch_group_setup(reinterpret_cast<const TmGroupSetup *>(D + o_su), reinterpret_cast<const int32_t *>(D + o_su_pre),
                                   (int)su.size(), su_pre.back(), lds_su, g->stream);
    }
    if (hr == 0 && !fu.empty()) {
        what = "group fused";
        hr = tm_launch_group_fused(reinterpret_cast<const TmGroupFused *>(D + o_fu), reinterpret_cast<const int32_t *>(D + o_fu_pre),
                                   (int)fu.size(), fu_pre.back(), lds_fu, g->stream);
    }
    for (int gen = 0; gen < 2 && hr == 0; gen++) {
        if (ev[gen].empty()) continue;
        what = "group eval";
        hr = tm_launch_group_eval(reinterpret_cast<const TmEvalArgs *>(D + o_ev[gen]), reinterpret_cast<const int32_t *>(D + o_ev_pre[gen]),
                                  reinterpret_cast<const int32_t *>(D + o_ev_nch[gen]), (int)ev[gen].size(), ev_pre[gen].back(),
                                  gen == 1, g->stream);
    }
    if (hr != 0) {
        rc = tm_launch_failed(what, hr);
        for (int k = 0; k < n; k++)
            if (Nchains[k] > 0) tm_zero_tickets(g->m[k], Nchains[k], g->stream);
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
    const int rc = tm_wait_slots(w, n, (size_t)n, [g]() {
        for (size_t k = 0; k < g->m.size(); k++) {
            const int nc = g->fl_off[k + 1] - g->fl_off[k];
            if (nc > 0) tm_zero_tickets(g->m[k], nc, g->stream);
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
    for (hipEvent_t *e : {&g->ev_after, &g->ev_done, &g->ev_tab[0], &g->ev_tab[1]})
        if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) return fail(TAMCMC_E_HIP);
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
    for (TmPinned *b : {&g->map[0], &g->map[1], &g->h_tab[0], &g->h_tab[1], &g->stage}) b->release();
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
    int rc = group_check(g, Nchains, Nparams);
    if (rc != TAMCMC_OK) return rc;
    if (!d_params || !d_Tcoefs || !d_logL) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(g->device));
    return group_enqueue(g, Nchains, d_params, d_Tcoefs, d_logL, d_status);
}

extern "C" int tamcmc_group_eval(tamcmc_group *g, const int32_t *Nchains, const int32_t *Nparams, const double *params,
                                 const double *Tcoefs, double *logL, int32_t *status)
{
    int rc = group_check(g, Nchains, Nparams);
    if (rc != TAMCMC_OK) return rc;
    if (!params || !Tcoefs || !logL) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(g->device));
    size_t np = 0, nc = 0;
    for (size_t k = 0; k < g->m.size(); k++) { np += (size_t)Nchains[k] * (size_t)Nparams[k]; nc += (size_t)Nchains[k]; }
    // staging [params | Tcoefs | logL | status]: one copy in, one copy out
    const size_t o_out = (np + nc) * sizeof(double), bytes_out = nc * (sizeof(double) + sizeof(int32_t)), bytes = o_out + bytes_out;
    if (!g->stage.fits(bytes)) {
        TM_HIP(hipStreamSynchronize(g->stream));
        rc = g->stage.reserve(bytes, TM_PIN_TWIN);
        if (rc != TAMCMC_OK) return rc;
    }
    char *const h_stage = g->stage.h, *const d_stage = g->stage.d;
    tm_stage_inputs(h_stage, params, np, Tcoefs, nc);
    // from here on, a failure waits for the stream before it returns: a copy from or into h_stage may still be pending,
    // and the next call refills it
    auto fail = [&](int code) { (void)hipStreamSynchronize(g->stream); return code; };
    hipError_t e = hipMemcpyAsync(d_stage, h_stage, o_out, hipMemcpyHostToDevice, g->stream);
    if (e != hipSuccess) { snprintf(tm_hip_err, sizeof(tm_hip_err), "group input copy -> %s", hipGetErrorString(e)); return fail(TAMCMC_E_HIP); }
    double *d_in = reinterpret_cast<double *>(d_stage);
    double *d_logL = reinterpret_cast<double *>(d_stage + o_out);
    int32_t *d_status = reinterpret_cast<int32_t *>(d_stage + o_out + nc * sizeof(double));
    rc = group_enqueue(g, Nchains, d_in, d_in + np, d_logL, d_status);
    if (rc != TAMCMC_OK) return fail(rc);
    e = hipMemcpyAsync(h_stage + o_out, d_stage + o_out, bytes_out, hipMemcpyDeviceToHost, g->stream);
    if (e == hipSuccess) e = hipEventRecord(g->ev_done, g->stream);
    if (e != hipSuccess) { snprintf(tm_hip_err, sizeof(tm_hip_err), "group output copy -> %s", hipGetErrorString(e)); return fail(TAMCMC_E_HIP); }
    rc = tm_poll_event(g->ev_done);
    if (rc != TAMCMC_OK) return fail(rc);
    std::memcpy(logL, h_stage + o_out, nc * sizeof(double));
    if (status) std::memcpy(status, h_stage + o_out + nc * sizeof(double), nc * sizeof(int32_t));
    return TAMCMC_OK;
}

// The host-pointer call in two halves, on mapped memory: no copy-engine transfer and no event on the way of a healthy call.
extern "C" int tamcmc_group_eval_begin(tamcmc_group *g, const int32_t *Nchains, const int32_t *Nparams, const double *params,
                                       const double *Tcoefs)
{
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
    if (!g->map[p].fits(bytes)) {
        TM_HIP(hipStreamSynchronize(g->stream));       // (a launch of two calls ago may not have retired yet)
        rc = g->map[p].reserve(bytes + bytes / 2, TM_PIN_MAPPED);
        if (rc != TAMCMC_OK) return rc;
    }
    char *h = g->map[p].h, *dv = g->map[p].d;
    tm_stage_inputs(h, params, np, Tcoefs, nc);
    g->fl_out = reinterpret_cast<uint64_t *>(h + o_out);
    g->fl_st = reinterpret_cast<int32_t *>(h + o_out + nc * sizeof(double));
    const TmWatch w{g->fl_out, g->fl_st, &g->ev_done, &g->ev_recorded, g->stream};
    tm_mark_slots(w, (int)nc, nc);
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
    return tm_poll_slot(g->fl_out, g->fl_st, (size_t)(o + chain), logL, status);
}

extern "C" int tamcmc_group_members(const tamcmc_group *g, int32_t *n_members, int32_t *Nparams, int32_t *device)
{
    if (!g) return TAMCMC_E_INVALID;
    if (n_members) *n_members = (int32_t)g->m.size();
    if (Nparams) for (size_t k = 0; k < g->m.size(); k++) Nparams[k] = g->m[k]->L.Nparams;
    if (device) *device = g->device;
    return TAMCMC_OK;
}
