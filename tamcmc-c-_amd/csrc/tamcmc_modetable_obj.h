// tamcmc_modetable_obj.h -- internal to csrc/: the posterior mode table's object, shared by the source files that work on
// it: tamcmc_modetable_api.cpp (the table, its statistics and quantiles), tamcmc_modediag_api.cpp (ESS, MCSE, split
// R-hat, covariances and correlations of its columns), tamcmc_moderank_api.cpp (their rank-normalised counterparts),
// tamcmc_seismic_api.cpp (the seismic indices appended to its columns) and tamcmc_modepdf_api.cpp (histograms, shortest
// intervals and pair densities of its columns).
#pragma once
#include "tamcmc_host.h"
#include "tamcmc_modetable.h"
#include "tamcmc_seismic.h"

struct tamcmc_modetable {
    tamcmc_ctx *c = nullptr;
    bool counted = false;                // the context's count includes this object
    int n_cols = 0, B = 0;
    long long max_samples = 0;
    std::vector<TmMtCol> cols;
    double *d_params = nullptr;          // [B][Nparams]
    double *d_rows = nullptr;            // [B][n_cols]
    int32_t *d_status = nullptr, *d_accept = nullptr;   // [B]
    double *d_state = nullptr;           // [TM_MT_NSTATE][n_cols], then the copy a push can be undone from, then [TM_Q_MAXQ][n_cols] quantiles
    uint64_t *d_ranks = nullptr;         // [TM_Q_MAXQ]
    double *d_table = nullptr;           // [n_cols][max_samples]
    long long n_used = 0, n_rejected = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms = 0.0;                     // derive and fold kernels since create / reset
    int64_t launches = 0;
    size_t state_doubles() const { return (size_t)TM_MT_NSTATE * (size_t)n_cols; }
    // tamcmc_modediag_* (tamcmc_modediag_api.cpp); nothing below is allocated before the first call that needs it
    double *d_acc = nullptr;             // [acc_lags][n_cols] lag products, then [TM_MD_NFIN][n_cols] tau, ess, rhat
    int32_t *d_cut = nullptr;            // [n_cols]
    int acc_lags = 0;                    // lags (L + 1) d_acc has room for
    int diag_L = 0;                      // L of the last _ess call, while acov_valid
    bool acov_valid = false;             // d_acc holds the lag products of the table as it is: no push or reset since
    double *d_S = nullptr;               // [sel_cap][sel_cap] sums of products of the last _cov / _corr call
    int32_t *d_sel = nullptr;            // [sel_cap] its columns
    int sel_cap = 0;
    double diag_ms = 0.0;                // lag, finish and covariance kernels since create / reset
    int64_t diag_launches = 0;
    // tamcmc_moderank_* (tamcmc_moderank_api.cpp); nothing below is allocated before the first call that needs it
    void *d_rk = nullptr;                // a chunk's key buffers, series, means, lag products, finish arrays (tmr_col_bytes each column)
    size_t rk_bytes = 0;                 // its size
    std::vector<double> rk_acov;         // [TM_MR_NSERIES][rk_L + 1][rk_nsel] lag products of the last _diag call, on the host
    int rk_L = 0, rk_nsel = 0;
    bool rk_valid = false;               // rk_acov is that of the table as it is: no push or reset since
    double rk_ms = 0.0;                  // sort, transform, mean, lag and finish kernels of _diag / _series since create / reset
    int64_t rk_launches = 0;
    // tamcmc_modetable_indices_* (tamcmc_seismic_api.cpp); n_index_cols = 0 and nothing below allocated until _indices_enable
    int n_base_cols = 0, n_index_cols = 0;          // n_cols = n_base_cols + n_index_cols
    TmSeisPlan plan;
    int32_t *d_seis_i = nullptr;         // first [n_index + 1], n_num [n_index], src [n_terms], wsrc [n_terms]
    double *d_seis_d = nullptr;          // coef [n_terms], offset [n_index]
    hipEvent_t seis_ev[2] = {nullptr, nullptr};
    double seis_ms = 0.0;                // indices kernel since create / reset
    int64_t seis_launches = 0;
    // tamcmc_modepdf_* (tamcmc_modepdf_api.cpp); nothing below is allocated before the first call that needs it
    void *d_pdf = nullptr;               // a call's arguments and counters, or an HPD chunk's keys and results
    size_t pdf_bytes = 0;                // its size
    double pdf_ms = 0.0;                 // histogram, pair and HPD kernels and the sort launches of _hpd since create / reset
    int64_t pdf_launches = 0;
};

// tamcmc_seismic_api.cpp, called by a block of tamcmc_modetable_derive / _push behind the derive kernel when n_index_cols > 0:
// the indices kernel on the block's n rows (between the object's seis_ev events when `timed`), and the addition of that time
// once the stream has been waited for.
int tm_seis_block(tamcmc_modetable *mt, int n, bool timed);
int tm_seis_timed_done(tamcmc_modetable *mt);
