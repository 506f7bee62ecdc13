// tamcmc_lockstep.cpp -- the lockstep evaluator of include/tamcmc_sampler.h: K samplers, each running its own loop on a
// host thread of its own, share ONE evaluation call per iteration (a fit group's launch, or any backend of that shape).
//
// Round protocol.  A member deposits its batch (pointers only), goes on with whatever does not need the results, then
// collects.  Deposits gather in the open round; the round fires when every JOINED member has deposited -- the thread
// that completes it (the last depositor, or a member that leaves) concatenates the blocks and makes the one call.  A
// member deposits into round r+1 only after it has collected round r, so when r+1 is complete round r has been collected
// by all its participants and closed: one round is in flight at any time, and all backend calls are made under the
// object's lock, one after the other.  Nobody holds the lock while waiting: a member waits for its round to fire by
// watching a counter (pauses, then yields, then short sleeps), and with a group backend it watches its own result slots
// (tamcmc_group_eval_poll) the same way the solo sampler does.
//
// Host-only C++ (g++): the group backend goes through the C ABI of tamcmc_accel.h.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "tamcmc_sampler.h"

namespace {

struct Member {
    bool joined = false;
    bool in_next = false;          // deposited into the open round
    bool in_cur = false;           // takes part in the fired round and has not collected yet
    int32_t nch = 0;
    const double *P = nullptr, *T = nullptr;
    double *outL = nullptr;
    int32_t *outS = nullptr;
    size_t off = 0;                // first slot of its block in the fired round
    uint64_t round = 0;            // the round it last deposited into
};

inline void relax_wait(unsigned &spins)
{
    ++spins;
    if (spins < 4096u) { __builtin_ia32_pause(); return; }
    if (spins < 8192u) { std::this_thread::yield(); return; }
    std::this_thread::sleep_for(std::chrono::microseconds(50));
}

} // namespace

struct tamcmc_lockstep {
    int n = 0;
    std::vector<int32_t> Nparams;
    tamcmc_group_eval_fn eval = nullptr;
    void *user = nullptr;
    tamcmc_group *group = nullptr;     // backend = the group's begin / end / poll
    std::mutex mu;
    std::vector<Member> mem;
    int n_joined = 0, n_dep = 0, n_uncollected = 0;
    uint64_t open_round = 0;           // id of the round that is gathering deposits
    std::atomic<uint64_t> fired{0};    // rounds fired so far (the call has returned)
    // the fired round
    std::vector<int32_t> Nch;
    std::vector<double> cat_P, cat_T, cat_L;
    std::vector<int32_t> cat_S;
    std::atomic<int> cur_rc{TAMCMC_OK};
    bool ended = true;                 // its results are final in cat_L / cat_S (or it failed)
    char err[256] = "";                // text of the last failed round
    int64_t calls = 0;
};

static void keep_error(tamcmc_lockstep *ls, int rc, const char *where)
{
    const char *h = (rc == TAMCMC_E_HIP) ? tamcmc_last_hip_error() : "";   // (thread-local in the library: this thread made the call)
    snprintf(ls->err, sizeof(ls->err), "%s: %s%s%s", where, tamcmc_strerror(rc), h[0] ? ": " : "", h);
}

// Lock held.  Fires the open round when every joined member has deposited.
static void try_fire(tamcmc_lockstep *ls)
{
    if (ls->n_dep < 1 || ls->n_dep != ls->n_joined || ls->n_uncollected != 0) return;
    size_t np = 0, nc = 0;
    for (int k = 0; k < ls->n; k++) {
        Member &m = ls->mem[(size_t)k];
        ls->Nch[(size_t)k] = m.in_next ? m.nch : 0;
        np += (size_t)ls->Nch[(size_t)k] * (size_t)ls->Nparams[(size_t)k];
        nc += (size_t)ls->Nch[(size_t)k];
    }
    ls->cat_P.resize(np); ls->cat_T.resize(nc); ls->cat_L.resize(nc); ls->cat_S.resize(nc);
    size_t po = 0, co = 0;
    for (int k = 0; k < ls->n; k++) {
        Member &m = ls->mem[(size_t)k];
        if (!m.in_next) continue;
        const size_t pk = (size_t)m.nch * (size_t)ls->Nparams[(size_t)k];
        std::memcpy(ls->cat_P.data() + po, m.P, pk * sizeof(double));
        std::memcpy(ls->cat_T.data() + co, m.T, (size_t)m.nch * sizeof(double));
        m.off = co;
        m.in_next = false; m.in_cur = true;
        po += pk; co += (size_t)m.nch;
    }
    ls->n_uncollected = ls->n_dep;
    ls->n_dep = 0;
    ls->calls++;
    int rc;
    if (ls->group) {
        rc = tamcmc_group_eval_begin(ls->group, ls->Nch.data(), ls->Nparams.data(), ls->cat_P.data(), ls->cat_T.data());
        ls->ended = (rc != TAMCMC_OK);             // (nothing in flight after a refused _begin)
        if (rc != TAMCMC_OK) keep_error(ls, rc, "tamcmc_group_eval_begin");
    } else {
        rc = ls->eval(ls->user, ls->n, ls->Nch.data(), ls->Nparams.data(), ls->cat_P.data(), ls->cat_T.data(), ls->cat_L.data(),
                      ls->cat_S.data());
        ls->ended = true;
        if (rc != TAMCMC_OK) keep_error(ls, rc, "lockstep backend");
    }
    ls->cur_rc = rc;
    ls->open_round++;
    ls->fired.store(ls->open_round, std::memory_order_release);
}

// Lock held.  Group backend: closes the batch in flight (exactly one thread gets here with ended == false).
static void close_round(tamcmc_lockstep *ls)
{
    if (ls->ended) return;
    const int rc = tamcmc_group_eval_end(ls->group, ls->cat_L.data(), ls->cat_S.data());
    ls->ended = true;
    if (rc != TAMCMC_OK) { ls->cur_rc = rc; keep_error(ls, rc, "tamcmc_group_eval_end"); }
}

static int lockstep_alloc(tamcmc_lockstep **out, int32_t n_members, const int32_t *Nparams)
{
    tamcmc_lockstep *ls = new (std::nothrow) tamcmc_lockstep();
    if (!ls) return TAMCMC_E_NOMEM;
    ls->n = n_members;
    ls->Nparams.assign(Nparams, Nparams + n_members);
    ls->mem.resize((size_t)n_members);
    ls->Nch.assign((size_t)n_members, 0);
    *out = ls;
    return TAMCMC_OK;
}

extern "C" int tamcmc_lockstep_create(tamcmc_lockstep **out, int32_t n_members, const int32_t *Nparams, tamcmc_group_eval_fn eval,
                                      void *user)
{
    if (!out) return TAMCMC_E_INVALID;
    *out = nullptr;
    if (n_members < 1 || n_members > 65536 || !Nparams || !eval) return TAMCMC_E_INVALID;
    for (int k = 0; k < n_members; k++) if (Nparams[k] < 1) return TAMCMC_E_INVALID;
    const int rc = lockstep_alloc(out, n_members, Nparams);
    if (rc == TAMCMC_OK) { (*out)->eval = eval; (*out)->user = user; }
    return rc;
}

extern "C" int tamcmc_lockstep_create_group(tamcmc_lockstep **out, tamcmc_group *g)
{
    if (!out) return TAMCMC_E_INVALID;
    *out = nullptr;
    if (!g) return TAMCMC_E_INVALID;
    int32_t n = 0;
    if (tamcmc_group_members(g, &n, nullptr, nullptr) != TAMCMC_OK || n < 1) return TAMCMC_E_INVALID;
    std::vector<int32_t> np((size_t)n);
    if (tamcmc_group_members(g, nullptr, np.data(), nullptr) != TAMCMC_OK) return TAMCMC_E_INVALID;
    const int rc = lockstep_alloc(out, n, np.data());
    if (rc == TAMCMC_OK) (*out)->group = g;
    return rc;
}

extern "C" int tamcmc_lockstep_join(tamcmc_lockstep *ls, int32_t member)
{
    if (!ls || member < 0 || member >= ls->n) return TAMCMC_E_INVALID;
    std::lock_guard<std::mutex> lk(ls->mu);
    Member &m = ls->mem[(size_t)member];
    if (m.joined) return TAMCMC_E_INVALID;
    m.joined = true;
    ls->n_joined++;
    return TAMCMC_OK;
}

extern "C" int tamcmc_lockstep_leave(tamcmc_lockstep *ls, int32_t member)
{
    if (!ls || member < 0 || member >= ls->n) return TAMCMC_E_INVALID;
    std::lock_guard<std::mutex> lk(ls->mu);
    Member &m = ls->mem[(size_t)member];
    if (!m.joined || m.in_next || m.in_cur) return TAMCMC_E_INVALID;   // (a round it has deposited into: collect first)
    m.joined = false;
    ls->n_joined--;
    try_fire(ls);                      // the others may have been waiting for this member only
    return TAMCMC_OK;
}

extern "C" int tamcmc_lockstep_destroy(tamcmc_lockstep *ls)
{
    if (!ls) return TAMCMC_OK;
    {
        std::lock_guard<std::mutex> lk(ls->mu);
        if (ls->n_joined > 0) return TAMCMC_E_INVALID;
    }
    delete ls;
    return TAMCMC_OK;
}

extern "C" const char *tamcmc_lockstep_error(const tamcmc_lockstep *ls) { return ls ? ls->err : ""; }

extern "C" int32_t tamcmc_lockstep_nparams(const tamcmc_lockstep *ls, int32_t member)
{
    return (ls && member >= 0 && member < ls->n) ? ls->Nparams[(size_t)member] : -1;
}

extern "C" int64_t tamcmc_lockstep_calls(const tamcmc_lockstep *ls) { return ls ? ls->calls : -1; }

extern "C" int tamcmc_lockstep_deposit(tamcmc_lockstep *ls, int32_t member, int32_t Nchains, int32_t Nparams, const double *params,
                                       const double *Tcoefs, double *logL, int32_t *status)
{
    if (!ls || member < 0 || member >= ls->n || Nchains < 1 || !params || !Tcoefs || !logL || !status) return TAMCMC_E_INVALID;
    if (Nparams != ls->Nparams[(size_t)member]) return TAMCMC_E_INVALID;
    std::lock_guard<std::mutex> lk(ls->mu);
    Member &m = ls->mem[(size_t)member];
    if (!m.joined || m.in_next || m.in_cur) return TAMCMC_E_INVALID;
    m.nch = Nchains; m.P = params; m.T = Tcoefs; m.outL = logL; m.outS = status;
    m.in_next = true;
    m.round = ls->open_round;
    ls->n_dep++;
    try_fire(ls);
    return TAMCMC_OK;
}

extern "C" int tamcmc_lockstep_collect(tamcmc_lockstep *ls, int32_t member)
{
    if (!ls || member < 0 || member >= ls->n) return TAMCMC_E_INVALID;
    Member &m = ls->mem[(size_t)member];
    {
        std::lock_guard<std::mutex> lk(ls->mu);
        if (!m.joined || !(m.in_next || m.in_cur)) return TAMCMC_E_INVALID;
    }
    // 1. the round fires when the last joined member has deposited (nobody holds the lock meanwhile)
    unsigned spins = 0;
    while (ls->fired.load(std::memory_order_acquire) <= m.round) relax_wait(spins);
    // 2. group backend: watch this member's own slots; bounded, _end (below) is what reports a failed launch
    bool have = false;
    if (ls->group && ls->cur_rc.load() == TAMCMC_OK) {
        have = true;
        long patience = 1L << 20;
        for (int32_t c = 0; c < m.nch && have; c++) {
            for (;;) {
                const int rp = tamcmc_group_eval_poll(ls->group, member, c, m.outL + c, m.outS + c);
                if (rp == TAMCMC_OK) break;
                if (rp != TAMCMC_PENDING || --patience < 0) { have = false; break; }   // (closed by another member, or slow)
                for (int b = 0; b < 8; b++) __builtin_ia32_pause();
            }
        }
    }
    // 3. hand in; the last collector closes the round, and so does one whose slots did not fill in time
    std::lock_guard<std::mutex> lk(ls->mu);
    if (!have || ls->n_uncollected == 1) close_round(ls);
    const int rc = ls->cur_rc.load();
    if (rc == TAMCMC_OK && !have) {
        std::memcpy(m.outL, ls->cat_L.data() + m.off, (size_t)m.nch * sizeof(double));
        std::memcpy(m.outS, ls->cat_S.data() + m.off, (size_t)m.nch * sizeof(int32_t));
    }
    m.in_cur = false;
    ls->n_uncollected--;
    try_fire(ls);
    return rc;
}
