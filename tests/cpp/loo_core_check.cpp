// loo_core_check -- the per-bin arithmetic of PSIS-LOO (tamcmc-c-_amd/csrc/tamcmc_loo.h) on the CPU, with the header's own
// functions: the rule for M, the top-(M+1) structure against a sort, and steps 3-4 (Pareto fit, smoothed tail, elpd_loo)
// with a single lane against a plain long-double transcription of the definition in include/tamcmc_accel.h.
//   g++ -std=c++17 -O1 -I tamcmc-c-_amd/csrc tests/cpp/loo_core_check.cpp -o loo_core_check && ./loo_core_check
// Prints one `ok` line; any failure prints what failed and exits 1.  (tests/test_summary_loo_host.py builds and runs it.)
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "tamcmc_loo.h"

static int failures = 0;
#define CHECK(cond, ...)                                                            \
    do {                                                                            \
        if (!(cond)) {                                                              \
            if (failures++ < 20) { fprintf(stderr, "FAILED %s:%d: %s  ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
        }                                                                           \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform()          // (0, 1)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(rng_state >> 11) + 0.5) / 9007199254740992.0;
}

static long check_M()
{
    long checked = 0;
    for (int64_t n = 1; n <= 30; n++, checked++)                 // n / 5 < 3 sqrt(n) up to n = 225: M = ceil(n / 5)
        CHECK(tml_tail_M(n) == (n + 4) / 5, "M(%lld) = %lld", (long long)n, (long long)tml_tail_M(n));
    CHECK(tml_tail_M(1) == 1 && tml_tail_M(20) == 4 && tml_tail_M(21) == 5, "M at 1, 20, 21");
    CHECK(tml_tail_M(70001) == 794, "M(70001) = %lld", (long long)tml_tail_M(70001));
    CHECK(tml_tail_M(466033) == TM_LOO_MAX_TAIL, "M(466033) = %lld", (long long)tml_tail_M(466033));
    CHECK(tml_tail_M(466034) == TM_LOO_MAX_TAIL + 1, "M(466034) = %lld", (long long)tml_tail_M(466034));
    return checked + 5;
}

// One column of n values pushed into a heap of `cap` slots at `stride`, the other columns of the buffer left alone.
static void check_column(const std::vector<double> &x, int cap, const char *what)
{
    const size_t stride = 3, col = 1;
    const int n = (int)x.size();
    const double guard = -12345.0;
    std::vector<double> buf((size_t)cap * stride, guard);
    double root = 0.0, a = 0.0, r = 0.0, c = 0.0;
    for (int s = 0; s < n; s++) tml_top_push(buf.data() + col, stride, cap, (long long)s, x[(size_t)s], &root, &a, &r, &c);
    const int cnt = n < cap ? n : cap;
    for (size_t k = 0; k < buf.size(); k++)
        if (k % stride != col || (int)(k / stride) >= cnt) CHECK(buf[k] == guard, "%s n=%d: a slot outside the column's first %d was written", what, n, cnt);
    std::vector<double> got, want(x);
    for (int k = 0; k < cnt; k++) got.push_back(buf[(size_t)k * stride + col]);
    for (int k = 1; k < cnt; k++) CHECK(!(got[(size_t)k] < got[(size_t)(k - 1) / 2]), "%s n=%d: heap order broken at slot %d", what, n, k);
    CHECK(root == got[0], "%s n=%d: the register root is not slot 0", what, n);
    std::sort(got.begin(), got.end());
    std::sort(want.begin(), want.end());
    for (int k = 0; k < cnt; k++) CHECK(got[(size_t)k] == want[(size_t)(n - cnt + k)], "%s n=%d cap=%d: value %d of the top set", what, n, cap, k);
    CHECK(root == want[(size_t)(n - cnt)], "%s n=%d: root", what, n);
    // the body: the n - cnt smallest, as a log-sum-exp
    if (n > cnt) {
        long double sum = 0.0L;
        const double top = want[(size_t)(n - cnt - 1)];
        for (int k = 0; k < n - cnt; k++) sum += expl((long double)want[(size_t)k] - (long double)top);
        const long double lse = (long double)top + logl(sum), mine = (long double)a + logl((long double)r - (long double)c);
        CHECK(fabsl(lse - mine) <= 1e-13L * (1.0L + fabsl(lse)), "%s n=%d: body log-sum-exp %.17Lg against %.17Lg", what, n, mine, lse);
    } else CHECK(r == 0.0, "%s n=%d: a body without members", what, n);
}

static long check_top()
{
    long checked = 0;
    for (int n = 1; n <= 300; n++) {
        std::vector<double> rnd, ties, desc, zeros;
        for (int s = 0; s < n; s++) {
            rnd.push_back(4.0 * uniform() - 2.0);
            ties.push_back((double)((int)(7.0 * uniform())) - 3.0);             // 7 distinct values: ties everywhere
            desc.push_back((double)(n - s) * 0.25);                             // every sample is below the root
            zeros.push_back(s % 3 == 0 ? -0.0 : (s % 3 == 1 ? 0.0 : (s % 2 ? 1.0 : -1.0)));
        }
        const int caps[] = {(int)tml_tail_M(n) + 1, 2, 17};
        for (int cap : caps) {
            check_column(rnd, cap, "random");
            check_column(ties, cap, "ties");
            check_column(desc, cap, "descending");
            check_column(zeros, cap, "zeros");
            std::vector<double> asc(desc.rbegin(), desc.rend());                // every sample replaces the root
            check_column(asc, cap, "ascending");
            checked += 5;
        }
    }
    return checked;
}

struct OneLane {
    int lane() const { return 0; }
    int lanes() const { return 1; }
    double sum(double v) const { return v; }
    void sync() const {}
};

struct Ref { long double elpd, khat, cutoff; int L; };

// the definition, transcribed
static Ref reference(const std::vector<double> &xs)
{
    const long n = (long)xs.size();
    const long double inf = std::numeric_limits<long double>::infinity();
    std::vector<long double> z(xs.begin(), xs.end());
    std::sort(z.begin(), z.end());
    const long double xmax = z.back();
    for (auto &v : z) v -= xmax;
    const long M = (long)tml_tail_M(n);
    Ref out{0.0L, inf, std::numeric_limits<long double>::quiet_NaN(), 0};
    long double c = inf;
    if (n > M) {
        out.cutoff = z[(size_t)(n - M - 1)] + xmax;
        c = std::max(z[(size_t)(n - M - 1)], logl((long double)DBL_MIN));
    }
    std::vector<long double> tail, body;
    for (auto v : z) (v > c ? tail : body).push_back(v);
    const long L = (long)tail.size();
    out.L = (int)L;
    std::vector<long double> zt(tail);
    if (L >= 5) {
        const long double ec = expl(c), dL = (long double)L;
        std::vector<long double> t;
        for (auto v : tail) t.push_back(expl(v) - ec);
        const long m = 30 + (long)floorl(sqrtl(dL)), q = (long)floorl(dL / 4.0L + 0.5L);
        std::vector<long double> th, ell, w;
        auto kof = [&](long double theta) { long double s = 0.0L; for (auto v : t) s += log1pl(-theta * v); return s / dL; };
        for (long j = 1; j <= m; j++) {
            th.push_back((1.0L - sqrtl((long double)m / ((long double)j - 0.5L))) / (3.0L * t[(size_t)(q - 1)]) + 1.0L / t[(size_t)(L - 1)]);
            const long double k = kof(th.back());
            ell.push_back(dL * (logl(-th.back() / k) - k - 1.0L));
        }
        long double wsum = 0.0L, that = 0.0L;
        for (long j = 0; j < m; j++) {
            long double den = 0.0L;
            for (long i = 0; i < m; i++) den += expl(ell[(size_t)i] - ell[(size_t)j]);
            w.push_back(1.0L / den);
            if (w.back() < 10.0L * (long double)DBL_EPSILON) w.back() = 0.0L;
            wsum += w.back();
        }
        for (long j = 0; j < m; j++) that += w[(size_t)j] / wsum * th[(size_t)j];
        const long double k = kof(that), sigma = -k / that;
        out.khat = (dL * k + 5.0L) / (dL + 10.0L);
        if (std::isfinite(out.khat))
            for (long j = 1; j <= L; j++) {
                const long double lp = log1pl(-((long double)j - 0.5L) / dL);
                const long double inner = out.khat == 0.0L ? -sigma * lp : sigma / out.khat * expm1l(-out.khat * lp);
                zt[(size_t)(j - 1)] = std::min(logl(inner + ec), 0.0L);
            }
    }
    long double num = (long double)body.size(), den = 0.0L;
    for (auto v : body) den += expl(v);
    for (long j = 0; j < L; j++) { num += expl(zt[(size_t)j] - tail[(size_t)j]); den += expl(zt[(size_t)j]); }
    out.elpd = logl(num) - xmax - logl(den);
    return out;
}

// the header's route: the top set, its candidates sorted, tml_finalize with one lane
static TmlBin mine(const std::vector<double> &xs)
{
    const long long n = (long long)xs.size();
    const int cap = (int)tml_tail_M(n) + 1;
    std::vector<double> heap((size_t)cap), t((size_t)cap), theta(TM_LOO_MAX_THETA), ell(TM_LOO_MAX_THETA);
    double root = 0.0, a = 0.0, r = 0.0, c = 0.0;
    for (long long s = 0; s < n; s++) tml_top_push(heap.data(), 1, cap, s, xs[(size_t)s], &root, &a, &r, &c);
    const int cnt = n < cap ? (int)n : cap;
    std::vector<double> cand(heap.begin() + 1, heap.begin() + cnt);
    std::sort(cand.begin(), cand.end());
    OneLane w;
    return tml_finalize(w, cand.data(), cnt - 1, heap[0], n >= cap, n, a, r - c, t.data(), theta.data(), ell.data());
}

static long check_finalize()
{
    long checked = 0;
    const int sizes[] = {1, 2, 4, 20, 21, 26, 100, 400, 3000};
    for (int n : sizes)
        for (int heavy = 0; heavy < 3; heavy++, checked++) {
            std::vector<double> xs;
            for (int s = 0; s < n; s++) {                                        // -l of a bin: a few units, with a tail of growing weight
                const double u = uniform(), g = sqrt(-2.0 * log(uniform())) * cos(6.283185307179586 * u);
                xs.push_back(3.0 + (heavy == 0 ? 0.3 * g : heavy == 1 ? 1.5 * g : 0.5 * g * g * g));
            }
            const Ref ref = reference(xs);
            const TmlBin got = mine(xs);
            CHECK(got.tail_len == ref.L, "n=%d heavy=%d: L = %d against %d", n, heavy, (int)got.tail_len, ref.L);
            if (n == 1) CHECK(std::isnan(got.cutoff) && got.elpd_loo == -xs[0], "n = 1: no tail rule, elpd = l");
            else CHECK((long double)got.cutoff == ref.cutoff, "n=%d heavy=%d: cutoff %.17g", n, heavy, got.cutoff);
            if (n <= 20) CHECK(std::isinf(got.pareto_k) && got.pareto_k > 0 && std::isinf(ref.khat), "n=%d: k-hat must be +inf", n);
            else CHECK(fabsl((long double)got.pareto_k - ref.khat) <= 1e-9L, "n=%d heavy=%d: k-hat %.17g against %.17Lg", n, heavy, got.pareto_k, ref.khat);
            CHECK(fabsl((long double)got.elpd_loo - ref.elpd) <= 1e-11L * (1.0L + fabsl(ref.elpd)), "n=%d heavy=%d: elpd %.17g against %.17Lg", n, heavy,
                  got.elpd_loo, ref.elpd);
        }
    // an all-equal column: the cutoff ties with everything, L = 0, k-hat = +inf, elpd = -x
    {
        std::vector<double> xs(50, 2.75);
        const TmlBin got = mine(xs);
        CHECK(got.tail_len == 0 && std::isinf(got.pareto_k) && got.cutoff == 2.75 && got.elpd_loo == -2.75, "all-equal column: L=%d k=%g elpd=%.17g",
              (int)got.tail_len, got.pareto_k, got.elpd_loo);
        checked++;
    }
    // every value three times: ties at the cutoff are body
    {
        std::vector<double> xs;
        for (int s = 0; s < 41; s++) { const double v = 4.0 * uniform(); xs.push_back(v); xs.push_back(v); xs.push_back(v); }
        const Ref ref = reference(xs);
        const TmlBin got = mine(xs);
        CHECK(got.tail_len == ref.L && ref.L % 3 == 0 && ref.L < (int)tml_tail_M(123), "triples: L = %d against %d", (int)got.tail_len, ref.L);
        CHECK(fabsl((long double)got.pareto_k - ref.khat) <= 1e-9L && fabsl((long double)got.elpd_loo - ref.elpd) <= 1e-11L, "triples: k-hat / elpd");
        checked++;
    }
    return checked;
}

int main()
{
    const long a = check_M(), b = check_top(), c = check_finalize();
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("ok loo_core_check: %ld M rules, %ld columns against a sort, %ld fits against the definition\n", a, b, c);
    return 0;
}
