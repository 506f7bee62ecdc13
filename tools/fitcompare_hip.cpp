// fitcompare_hip -- compares up to eight fits of one spectrum from the files chainsummary_hip writes (tamcmc_compare_* in
// include/tamcmc_accel_compare.h).
//
//   fitcompare_hip <file_0> <file_1> [... up to 8] <result file> [--column NAME] [--scale s] [--bootstrap R[,seed]]
//                  [--stacking [tol[,max_iter]]]
//
// The input files are the output file of `chainsummary_hip --loo` (columns elpd_loo and pareto_k, leading columns x and y) or
// its .loowin file (elpd_lwo and pareto_k, leading columns first_bin and last_bin).  The columns are found by name in the last
// `#` line before the rows.  --column NAME takes another column as the pointwise value (lppd, say); the default is elpd_loo,
// or elpd_lwo where there is no elpd_loo.  Files whose row counts differ, or whose leading columns differ in any row, are
// refused: the fits must be of one spectrum on one grid or one set of windows.  file_0 is the reference fit of the bootstrap.
// --scale s: the log predictive density is s times the column (0.5 for the chi_square likelihood), default 1.
//
// The result file: `#` lines -- the version; `# fits= K  units= N  n_included= ...  n_excluded= ...  column= NAME  scale= s`;
// per pair a > b `# pair a b  elpd_diff= ...  se_diff= ...  n_better= ...  n_worse= ...  n_k_high= ...  diff_k_high= ...`;
// `# pseudo_bma= w_0 ... w_{K-1}`; with --bootstrap `# bootstrap R= ...  seed= ...`, per pair `# prob a b  n_greater= ...
// n_equal= ...  q05= ...  q95= ...` (the interval of z_a - z_b) and `# pseudo_bma_plus= ...`; with --stacking `# stacking= ...`
// and `# stacking_info iterations= ...  converged= ...  gap= ...  f= ...  tol= ...  max_iter= ...` -- then the column names and one
// row per unit: its leading columns and d_1 ... d_{K-1}, d_k = value of fit k minus value of fit 0.  <result file>.top holds
// per fit k >= 1 the 20 units of largest |d_k|, largest first: k, the unit's row, its leading columns and d_k.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "tamcmc_accel.h"

struct FitFile {
    std::vector<double> lead0, lead1, value, khat;
    std::string lead_name0, lead_name1;
    bool has_khat = false;
};

static int usage()
{
    fprintf(stderr, "Usage: fitcompare_hip <file_0> <file_1> [... up to 8] <result file> [--column NAME] [--scale s]\n"
                    "                      [--bootstrap R[,seed]] [--stacking [tol[,max_iter]]]\n"
                    "     <file_k>   the output file of chainsummary_hip --loo (x y ... elpd_loo pareto_k) or its .loowin file\n"
                    "                (first_bin last_bin ... elpd_lwo pareto_k); file_0 is the reference fit\n"
                    "     --column NAME   the pointwise value (default elpd_loo, or elpd_lwo)     --scale s   log density = s x value (default 1)\n"
                    "     --bootstrap R[,seed]   R replicates of the Bayesian bootstrap: prob, the 5 %% and 95 %% points, pseudo-BMA+ weights\n"
                    "     --stacking [tol[,max_iter]]   stacking weights (default 1e-8,100000)\n"
                    "     The result file: # lines with every pair's totals, the weights and the stacking info, then one row per unit with\n"
                    "     its leading columns and d_1 ... d_{K-1}; <result file>.top: the 20 units of largest |d| per fit\n");
    return 2;
}

static int fail(const std::string &msg)
{
    fprintf(stderr, "fitcompare_hip: %s\n", msg.c_str());
    return 1;
}

static bool parse_double(const std::string &s, double *v)
{
    if (s.empty()) return false;
    char *end = nullptr;
    *v = strtod(s.c_str(), &end);
    return end && *end == '\0';
}

static bool parse_u64(const std::string &s, unsigned long long *v)
{
    if (s.empty() || s[0] == '-' || s[0] == '+') return false;
    char *end = nullptr;
    *v = strtoull(s.c_str(), &end, 10);
    return end && *end == '\0';
}

static bool read_fit(const std::string &path, std::string column, FitFile *f, std::string *used, std::string *err)
{
    std::ifstream in(path);
    if (!in) { *err = "unable to read " + path; return false; }
    std::string line, names;
    std::vector<std::string> rows;
    while (std::getline(in, line)) {
        size_t p = line.find_first_not_of(" \t\r");
        if (p == std::string::npos) continue;
        if (line[p] == '#') { if (rows.empty()) names = line.substr(p + 1); continue; }
        rows.push_back(line);
    }
    std::vector<std::string> cols;
    { std::istringstream ss(names); std::string t; while (ss >> t) cols.push_back(t); }
    auto find = [&](const std::string &n) { for (size_t c = 0; c < cols.size(); c++) if (cols[c] == n) return (int)c; return -1; };
    if (column.empty()) column = find("elpd_loo") >= 0 ? "elpd_loo" : "elpd_lwo";
    const int cv = find(column), ck = find("pareto_k");
    if (cv < 0) { *err = path + ": no column " + column + " in the header line"; return false; }
    if (cols.size() < 2) { *err = path + ": fewer than two columns"; return false; }
    *used = column;
    f->lead_name0 = cols[0]; f->lead_name1 = cols[1];
    f->has_khat = ck >= 0;
    for (const std::string &r : rows) {
        std::istringstream ss(r);
        std::string t;
        std::vector<double> v;
        while (ss >> t) { double x; if (!parse_double(t, &x)) { *err = path + ": not a number: " + t; return false; } v.push_back(x); }
        if (v.size() != cols.size()) { *err = path + ": a row with " + std::to_string(v.size()) + " columns under " + std::to_string(cols.size()) + " names"; return false; }
        f->lead0.push_back(v[0]); f->lead1.push_back(v[1]); f->value.push_back(v[(size_t)cv]);
        if (ck >= 0) f->khat.push_back(v[(size_t)ck]);
    }
    if (rows.empty()) { *err = path + ": no rows"; return false; }
    return true;
}

int main(int argc, char **argv)
{
    std::vector<std::string> pos;
    std::string column;
    double scale = 1.0, tol = 1e-8;
    unsigned long long R = 0, seed = 0, max_iter = 100000;
    bool stacking = false, seen_boot = false, seen_col = false, seen_scale = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--column") {
            if (seen_col || i + 1 >= argc) return usage();
            seen_col = true; column = argv[++i];
            if (column.empty()) return usage();
        } else if (a == "--scale") {
            if (seen_scale || i + 1 >= argc || !parse_double(argv[++i], &scale) || !(scale > 0.0) || std::isinf(scale)) return usage();
            seen_scale = true;
        } else if (a == "--bootstrap") {
            if (seen_boot || i + 1 >= argc) return usage();
            seen_boot = true;
            const std::string v = argv[++i];
            const size_t c = v.find(',');
            if (!parse_u64(v.substr(0, c), &R) || R < 1 || R > TAMCMC_COMPARE_MAX_REPLICATES) return usage();
            if (c != std::string::npos && !parse_u64(v.substr(c + 1), &seed)) return usage();
        } else if (a == "--stacking") {
            if (stacking) return usage();
            stacking = true;
            // an optional value: what follows is taken as tol[,max_iter] if its first part parses as a number
            if (i + 1 < argc && argv[i + 1][0] != '\0' && strncmp(argv[i + 1], "--", 2) != 0 && strchr(argv[i + 1], '/') == nullptr) {
                double t;
                const std::string v = argv[i + 1];
                const size_t c = v.find(',');
                if (parse_double(v.substr(0, c), &t)) {
                    if (!(t >= 0.0) || std::isinf(t)) return usage();
                    if (c != std::string::npos && (!parse_u64(v.substr(c + 1), &max_iter) || max_iter < 1 || max_iter > (1ull << 24))) return usage();
                    tol = t;
                    i++;
                }
            }
        } else if (!a.empty() && a[0] == '-') {
            return usage();
        } else {
            pos.push_back(a);
        }
    }
    if (pos.size() < 3 || pos.size() > TAMCMC_COMPARE_MAX_FITS + 1) return usage();
    const int K = (int)pos.size() - 1;
    const std::string out_file = pos.back();

    std::vector<FitFile> fits((size_t)K);
    std::string used, err;
    for (int k = 0; k < K; k++) {
        std::string u;
        if (!read_fit(pos[(size_t)k], column, &fits[(size_t)k], &u, &err)) return fail(err);
        if (k == 0) used = u;
        else if (u != used) return fail(pos[(size_t)k] + ": column " + u + ", but " + pos[0] + " has " + used);
    }
    const size_t N = fits[0].value.size();
    bool khat = true;
    for (int k = 0; k < K; k++) {
        const FitFile &f = fits[(size_t)k];
        if (f.value.size() != N) return fail(pos[(size_t)k] + ": " + std::to_string(f.value.size()) + " rows, but " + pos[0] + " has " + std::to_string(N));
        if (f.lead_name0 != fits[0].lead_name0 || f.lead_name1 != fits[0].lead_name1) return fail(pos[(size_t)k] + ": other leading columns than " + pos[0]);
        for (size_t i = 0; i < N; i++)
            if (f.lead0[i] != fits[0].lead0[i] || f.lead1[i] != fits[0].lead1[i])
                return fail(pos[(size_t)k] + ": row " + std::to_string(i) + " differs from " + pos[0] + " in its leading columns (another spectrum or grid)");
        khat = khat && f.has_khat;
    }
    std::vector<double> elpd((size_t)K * N), kh;
    for (int k = 0; k < K; k++) std::copy(fits[(size_t)k].value.begin(), fits[(size_t)k].value.end(), elpd.begin() + (size_t)k * N);
    if (khat) {
        kh.resize((size_t)K * N);
        for (int k = 0; k < K; k++) std::copy(fits[(size_t)k].khat.begin(), fits[(size_t)k].khat.end(), kh.begin() + (size_t)k * N);
    }

    tamcmc_compare *h = nullptr;
    auto lib_fail = [&](const char *where, int rc) {
        std::string m = std::string(where) + ": " + tamcmc_strerror(rc);
        if (rc == TAMCMC_E_HIP) m += std::string(" | ") + tamcmc_last_hip_error();
        if (h) tamcmc_compare_destroy(h);
        return fail(m);
    };
    int rc = tamcmc_compare_create(&h, 0, K, (int64_t)N, elpd.data(), khat ? kh.data() : nullptr, scale, seed, 0);
    if (rc != TAMCMC_OK) return lib_fail("tamcmc_compare_create", rc);
    int64_t n_inc = 0, n_exc = 0;
    tamcmc_compare_info(h, &n_inc, &n_exc);

    FILE *o = fopen(out_file.c_str(), "w");
    if (!o) { tamcmc_compare_destroy(h); return fail("unable to open the result file " + out_file); }
    fprintf(o, "# fitcompare_hip (%s)\n", tamcmc_version());
    fprintf(o, "# fits= %d  units= %zu  n_included= %lld  n_excluded= %lld  column= %s  scale= %.17g\n", K, N, (long long)n_inc, (long long)n_exc, used.c_str(), scale);
    for (int a = 1; a < K; a++)
        for (int b = 0; b < a; b++) {
            tamcmc_compare_totals t;
            rc = tamcmc_compare_diff(h, a, b, &t);
            if (rc != TAMCMC_OK) { fclose(o); return lib_fail("tamcmc_compare_diff", rc); }
            fprintf(o, "# pair %d %d  elpd_diff= %.17g  se_diff= %.17g  n_better= %lld  n_worse= %lld  n_k_high= %lld  diff_k_high= %.17g\n", a, b, t.elpd_diff,
                    t.se_diff, (long long)t.n_better, (long long)t.n_worse, (long long)t.n_k_high, t.diff_k_high);
        }
    double w[TAMCMC_COMPARE_MAX_FITS];
    auto put_w = [&](const char *name) {
        fprintf(o, "# %s=", name);
        for (int k = 0; k < K; k++) fprintf(o, " %.17g", w[k]);
        fprintf(o, "\n");
    };
    if (n_inc > 0) {
        rc = tamcmc_compare_weights(h, TAMCMC_COMPARE_PSEUDO_BMA, w);
        if (rc != TAMCMC_OK) { fclose(o); return lib_fail("tamcmc_compare_weights", rc); }
        put_w("pseudo_bma");
    }
    if (R > 0) {
        rc = tamcmc_compare_bootstrap(h, (int64_t)R, 0);
        if (rc != TAMCMC_OK) { fclose(o); return lib_fail("tamcmc_compare_bootstrap", rc); }
        fprintf(o, "# bootstrap R= %llu  seed= %llu\n", R, seed);
        for (int a = 1; a < K; a++)
            for (int b = 0; b < a; b++) {
                int64_t gt = 0, eq = 0;
                double q05 = 0.0, q95 = 0.0;
                rc = tamcmc_compare_prob(h, a, b, &gt, &eq);
                if (rc == TAMCMC_OK) rc = tamcmc_compare_interval(h, a, b, 0.05, &q05);
                if (rc == TAMCMC_OK) rc = tamcmc_compare_interval(h, a, b, 0.95, &q95);
                if (rc != TAMCMC_OK) { fclose(o); return lib_fail("tamcmc_compare_prob", rc); }
                fprintf(o, "# prob %d %d  n_greater= %lld  n_equal= %lld  q05= %.17g  q95= %.17g\n", a, b, (long long)gt, (long long)eq, q05, q95);
            }
        rc = tamcmc_compare_weights(h, TAMCMC_COMPARE_PSEUDO_BMA_PLUS, w);
        if (rc != TAMCMC_OK) { fclose(o); return lib_fail("tamcmc_compare_weights", rc); }
        put_w("pseudo_bma_plus");
    }
    if (stacking) {
        tamcmc_compare_stacking_info info;
        rc = tamcmc_compare_stacking(h, tol, (int64_t)max_iter, 0, w, &info);
        if (rc != TAMCMC_OK) { fclose(o); return lib_fail("tamcmc_compare_stacking", rc); }
        put_w("stacking");
        fprintf(o, "# stacking_info iterations= %lld  converged= %d  gap= %.17g  f= %.17g  tol= %.17g  max_iter= %llu\n", (long long)info.iterations,
                info.converged, info.gap, info.f, tol, max_iter);
    }
    tamcmc_compare_destroy(h);

    fprintf(o, "# %s %s", fits[0].lead_name0.c_str(), fits[0].lead_name1.c_str());
    for (int k = 1; k < K; k++) fprintf(o, " d_%d", k);
    fprintf(o, "\n");
    for (size_t i = 0; i < N; i++) {
        fprintf(o, "%.17g %.17g", fits[0].lead0[i], fits[0].lead1[i]);
        for (int k = 1; k < K; k++) fprintf(o, " %.17g", elpd[(size_t)k * N + i] - elpd[i]);
        fprintf(o, "\n");
    }
    if (fclose(o) != 0) return fail("unable to write the result file " + out_file);

    const std::string top_file = out_file + ".top";
    FILE *t = fopen(top_file.c_str(), "w");
    if (!t) return fail("unable to open the result file " + top_file);
    fprintf(t, "# fitcompare_hip (%s)\n# fit row %s %s d\n", tamcmc_version(), fits[0].lead_name0.c_str(), fits[0].lead_name1.c_str());
    for (int k = 1; k < K; k++) {
        std::vector<size_t> idx;
        for (size_t i = 0; i < N; i++) {
            bool ok = true;
            for (int j = 0; j < K; j++) ok = ok && std::isfinite(elpd[(size_t)j * N + i]);
            if (ok) idx.push_back(i);
        }
        const double *e0 = elpd.data(), *ek = elpd.data() + (size_t)k * N;
        std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return std::fabs(ek[x] - e0[x]) > std::fabs(ek[y] - e0[y]); });
        for (size_t m = 0; m < idx.size() && m < 20; m++)
            fprintf(t, "%d %zu %.17g %.17g %.17g\n", k, idx[m], fits[0].lead0[idx[m]], fits[0].lead1[idx[m]], ek[idx[m]] - e0[idx[m]]);
    }
    if (fclose(t) != 0) return fail("unable to write the result file " + top_file);
    return 0;
}
