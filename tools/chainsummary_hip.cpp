// chainsummary_hip -- posterior summaries of a stored chain on the GPU path (tamcmc_summary_* in tamcmc_accel.h): the
// posterior-mean model with its envelope and the WAIC terms, per bin, from the samples a run has written.
//
//   chainsummary_hip <config dir> <model file> <data file> <params root> <output file>
//                    [--chain m] [--slice s] [--first i] [--last j] [--thin k] [--block B]
//                    [--quantiles q1,q2,...] [--qbits b] [--loo] [--predictive] [--window W[,first]] [--ess [L]]
//                    [--scan W0[,W1,...]] [--scan-below T] [--scan-null R[,seed]] [--band-ess [L]] [--loo-pit]
//                    [--loo-window W[,first]] [--modes [q1,q2,...]] [--modes-ess [L]] [--modes-corr]
//                    [--modes-rank [L]] [--modes-indices] [--modes-hist [N]] [--modes-hpd m1[,m2,...]]
//                    [--modes-pairs c1:c2[,c3:c4,...] [N]]
//
// <config dir> is the reference's Config/default; model id, likelihood, p, plength, the inputs row and the relax mask
// come from the setup it describes (tamcmc_setup_create / tamcmc_setup_load, slice s counted from 0).  The samples are
// read from <params root>_chain-<m>.bin with Nvars from <params root>.hdr (written by tamcmc_outputs.cpp); every row of
// variables is scattered into the inputs row (Model_def::update_params_with_vars, model_def.cpp:370-378) -- the
// constants come from the .model file, not from the header's 6-digit constant_values.  Samples first, first + thin, ...
// up to last (both counted from 0, inclusive) are pushed in blocks of B (0: the library's default).
// Output: `#` header lines with the totals and the sample range, then the columns
//   x  y  mean_M  sd_M  min_M  max_M  lppd  var_l            (12 significant digits, like getmodel_hip)
// With --quantiles (up to 8 values in [0, 1]) the selected samples are read again once per pass of the exact quantile
// selection (tamcmc_summary_quantiles_*; b bits per pass, 0: the library's default), the header gains a line
// `# quantiles= q1,q2,...  passes= N`, and one column per quantile follows var_l: the order statistic of the model in that
// bin, numpy's "inverted_cdf".
// With --loo the selected samples are read once more for PSIS-LOO (tamcmc_summary_loo_*), the header gains a line
// `# elpd_loo= ...  p_loo= ...  looic= ...  k_max= ...  n_k_high= ...  n_k_inf= ...`, and two more columns follow the
// quantiles: elpd_loo and pareto_k, the bin's leave-one-out log predictive density and its Pareto k-hat (above 0.7: not to
// be trusted).
// With --loo-pit (implies --loo) the selected samples are read a third time for the leave-one-out PIT
// (tamcmc_summary_loo_pit_*): the predictive tails under the PSIS weights, and the weights' effective sample size.  The
// output file is that of --loo; the results go to <output file>.loopit: `#` header lines -- the version, `# n_used= ...
// n_rejected= ...`, `# ks_D= ...  min_log_sf= ...  bin_min_log_sf= ...  min_log_cdf= ...  bin_min_log_cdf= ...`,
// `# min_is_ess= ...  bin_min_is_ess= ...`, `# pit_hist= c0 c1 ... c19` -- then one row per bin:
//   x  loo_pit  loo_log_cdf  loo_log_sf  is_ess  pareto_k
// With --loo-window W[,first] the selected samples are read once more for leave-one-window-out PSIS-LOO over disjoint windows
// of W bins, the first window `first` bins long (tamcmc_summary_wloo_*), and with --loo-pit a further time for the LOO-PIT
// of every window.  The output file and the other files keep every byte; the results go to <output file>.loowin: `#` header
// lines -- the version, `# W= ...  first= ...  n_windows= ...`, `# n_used= ...  n_rejected= ...`, `# elpd_lwo= ...  p_lwo= ...
// k_max= ...  n_k_high= ...  n_k_inf= ...`, and with --loo-pit the three lines of .loopit's totals with windows for bins
// -- then one row per window:
//   first_bin  last_bin  x_first  x_last  elpd_lwo  pareto_k  tail_len  [loo_pit  loo_log_cdf  loo_log_sf  is_ess  log_wsum]
// With --predictive the first pass also accumulates the posterior predictive check (tamcmc_summary_predictive_*; no further
// pass), the header gains two lines, `# ks_D= ...  min_log_sf= ...  bin_min_log_sf= ...  min_log_cdf= ...
// bin_min_log_cdf= ...` and `# pit_hist= c0 c1 ... c19`, and four columns follow all the others: pit, log_cdf, log_sf and
// mean_resid -- the bin's probability integral transform, the logarithms of its two predictive tail probabilities (log_sf
// far below 0: power the model does not explain) and its mean residual.
// With --window W[,first] the first pass also accumulates the same check over disjoint windows of W bins, the first window
// `first` bins long (tamcmc_summary_window_*; no further pass).  The output file keeps every byte; the windows go to
// <output file>.windows: `#` header lines -- the version, `# W= ...  first= ...  n_windows= ...`, `# n_used= ...
// n_rejected= ...`, `# ks_D= ...  min_log_sf= ...  win_min_log_sf= ...  min_log_cdf= ...  win_min_log_cdf= ...`,
// `# pit_hist= c0 c1 ... c19` -- then one row per window:
//   w  first_bin  last_bin  x_first  x_last  pit  log_cdf  log_sf  mean_resid
// With --scan W0[,W1,...] (up to 8 strictly ascending widths) the first pass also accumulates that check at every start
// position j = 0 ... Nx - W of every width (tamcmc_summary_scan_*; no further pass).  The output file and .windows keep every
// byte; the scan goes to <output file>.scan: `#` header lines -- the version, `# widths= W0,W1,...`, `# n_used= ...
// n_rejected= ...`, per width `# W= ...  n_positions= ...  min_log_sf= ...  pos_min_log_sf= ...  min_log_cdf= ...
// pos_min_log_cdf= ...` -- then one row per bin j, 17 significant digits, `nan` where width k has no position j:
//   j  x_j  then for each width  pit  log_cdf  log_sf  mean_resid
// and the regions -- the maximal runs of positions whose log_sf (which = 0) or log_cdf (which = 1) lies below the line -- to
// <output file>.scan.regions, one row per region of either side, per width:
//   W  which  pos_first  pos_last  bin_first  bin_last  x_first  x_last  pos_min  min_log  mean_resid_at_min
// The line is T of --scan-below T (T < 0) for all widths, by default log(0.01 W / Nx) per width.
// With --scan-null R[,seed] (needs --scan; R replicates with floor(0.01 (R + 1)) >= 1, seed default 0) the null distribution of
// the scan's extremes is simulated on the device (tamcmc_scan_null_*): without --scan-below the regions' line becomes the
// joint 1 % line of each width and side.  .scan keeps every byte; .scan.regions gains one header line, `# null= R seed
// alpha= 0.01 joint_line= ...` (per width the excess side's line, then the deficit side's; `log_below=` lists the lines in
// use in the same order unless --scan-below set one for all), and two trailing columns, p_width and p_joint of min_log.
// With --ess [L] the selected samples are read once more for the effective sample size, the Monte-Carlo standard error and
// the split R-hat per bin (tamcmc_summary_ess_*; lags up to L, 0 ... 1023, default 0: the library's 255).  The output file
// keeps every byte; the results go to <output file>.ess: `#` header lines -- the version, `# n_used= ...  n_rejected= ...
// lag= ...`, `# min_ess_M= ...  bin_min_ess_M= ...  min_ess_l= ...  bin_min_ess_l= ...`, `# max_rhat= ...  bin_max_rhat= ...
// n_rhat_high= ...`, `# n_truncated_M= ...  n_truncated_l= ...` -- then one row per bin:
//   x  ess_M  tau_M  mcse_M  rhat_M  cut_M  ess_l  r_eff  cut_l
// With --band-ess [L] (needs --quantiles) the selected samples are read once more after the selection is exact, for the
// effective sample size of every quantile: that of the indicator `model <= quantile` (tamcmc_summary_bandess_*; lags up to L as
// for --ess).  The output file keeps every byte; the results go to <output file>.bandess: `#` header lines -- the version,
// `# quantiles= q1,q2,...`, `# n_used= ...  n_rejected= ...  lag= ...`, per quantile `# q= ...  min_ess= ...  bin_min_ess= ...
// n_truncated= ...  n_constant= ...` -- then one row per bin, x and per quantile seven columns:
//   value  count_le  p_hat  ess  tau  mcse_p  cut
// With --modes [q1,q2,...] the selected samples are read once more for the posterior mode table (tamcmc_modetable_*): the
// derived quantities of every multiplet and of the chain, their mean, sd, minimum, maximum and exact quantiles (default
// 0.16,0.5,0.84) over the samples the fold used.  The output file keeps every byte; the results go to <output file>.modes:
// `#` header lines -- the version, `# quantiles= q1,q2,...`, `# n_used= ...  n_rejected= ...  n_cols= ...  n_mult= ...` (the
// samples the fold skipped are counted among the rejected) and the column names -- then one row per quantity:
//   col  kind  mult  order  l  m  param_index  mean  sd  min  max  [one column per quantile]        (17 significant digits)
// With --modes-ess [L] (needs --modes; L as for --ess) the table's columns get their effective sample size, Monte-Carlo
// standard error and split R-hat (tamcmc_modediag_ess) from the rows the table already holds: <output file>.modes.ess, `#`
// header lines -- the version, the .modes totals, `# lag= ...  min_ess= ...  col_min_ess= ...  max_rhat= ...  col_max_rhat= ...
// n_truncated= ...  n_constant= ...  n_rhat_high= ...` and the column names -- then one row per quantity:
//   col  kind  mult  order  l  m  param_index  ess  tau  mcse  rhat  cut                             (17 significant digits)
// With --modes-corr (needs --modes) the correlation matrix of the headline columns -- the four chain-level columns and freq,
// width, height, amplitude, splitting of every multiplet, in table order -- goes to <output file>.modes.corr: the version, the
// .modes totals, `# cols = c0 c1 ...`, then the matrix, one row per line (17 significant digits; nan where a column is constant).
// With --modes-rank [L] (needs --modes; L as for --modes-ess) the table's columns get their rank-normalised diagnostics
// (tamcmc_moderank_diag): bulk and tail effective sample size, rank-normalised and folded split R-hat, to
// <output file>.modes.rank: the version, the .modes totals, `# lag= ...  min_ess_bulk= ...  col_min_ess_bulk= ...  min_ess_tail= ...
// col_min_ess_tail= ...  max_rhat= ...  col_max_rhat= ...  n_truncated= ...  n_constant= ...  n_rhat_high= ...`, the column names, then
// one row per quantity in the order of .modes.ess:
//   col  kind  mult  order  l  m  param_index  ess_bulk  ess_tail  rhat  tau_bulk  rhat_bulk  rhat_fold  ess_q05  ess_q95
//   cut_z  cut_zfold  cut_i05  cut_i95                                                               (17 significant digits)
// None of the three reads the samples again; the output file, .modes and .modes.ess keep every byte.
// With --modes-indices (needs --modes) the seismic indices (tamcmc_modetable_indices_enable: Dnu and epsilon of the radial
// ridge, nu_max, per-order separations and second differences, d02, d13, d01, d10, r02, r01, r13, r10) are computed per
// sample in a mode table of their own, whose reference row is the first selected sample the derivation accepts; the samples
// are read once more and every other file keeps every byte.  <output file>.modes.indices: the version, `# quantiles= ...`, `#
// n_used= ...  n_rejected= ...  n_base_cols= ...  n_index_cols= ...  n_radial= ...  n_unassigned= ...  n_base= ...  dnu_ref= ...
// eps_ref= ...`, the column names, then one row per index column:
//   col  kind  l  n  mean  sd  [one column per quantile]  [ess tau mcse rhat cut with --modes-ess]
//   [ess_bulk ess_tail rhat_rank tau_bulk rhat_bulk rhat_fold ess_q05 ess_q95 cut_z cut_zfold cut_i05 cut_i95 with --modes-rank]
// <output file>.modes.indices.cov: the covariance matrix (tamcmc_modediag_cov) of the ratio columns r02, r01, r13, r10 in
// column order: the version, the totals, `# cols = c0 c1 ...`, `# rows = r02_n<n> ...`, then one matrix row per line.  A
// star the plan refuses (fewer than 3 radial modes, a missing radial order), or a chain of which fewer than 2 samples (4 with
// --modes-ess or --modes-rank) are accepted with their indices, gets a message and neither file; every other file is written.
// With --modes-hist [N] (needs --modes; N classes, 1 ... 4096, default 50) the marginal histogram of every column of the
// table (tamcmc_modepdf_hist over the column's min ... max) goes to <output file>.modes.hist: the version, the .modes totals,
// `# n_bins= N`, then per column a block: `# col kind mult order l m param_index`, `# range= lo hi  status= s`, `# below= b
// above= a`, then N lines `edge count` (the class' lower plot edge, 17 significant digits) and a last line `hi` alone.  The
// edges are for plotting; the counts follow the library's class rule.
// With --modes-hpd m1[,m2,...] (needs --modes; up to 8 masses in (0, 1], at least 4 accepted samples) the shortest interval
// holding each mass (tamcmc_modepdf_hpd) goes to <output file>.modes.hpd: the version, the .modes totals, `# mass= m1,m2,...`,
// `# k= k1 k2 ...`, the column names, then one row per column:
//   col  kind  mult  order  l  m  param_index  median  [k lo hi per mass]                           (17 significant digits)
// With --modes-pairs c1:c2[,c3:c4,...] [N] (needs --modes; column indices of the table, N classes an axis, 1 ... 128, default
// 32) the joint histogram of each pair (tamcmc_modepdf_hist2d over the columns' min ... max) and its contour levels at 68 %
// and 95 % go to <output file>.modes.pairs: the version, the .modes totals, `# n_bins= N`, then per pair a block: `# pair c1
// c2`, `# range= lo1 hi1 lo2 hi2  status= s`, `# outside= o  level68= t  level95= t`, then N lines of N counts, the row the
// class of c1.  None of the three reads the samples again; every other file keeps every byte.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "tamcmc_accel.h"
#include "tamcmc_io.h"

static int usage()
{
    fprintf(stderr, " Usage: chainsummary_hip <config dir> <model file> <data file> <params root> <output file>\n"
                    "                         [--chain m] [--slice s] [--first i] [--last j] [--thin k] [--block B]\n"
                    "                         [--quantiles q1,q2,...] [--qbits b] [--loo] [--predictive] [--window W[,first]] [--ess [L]]\n"
                    "                         [--scan W0[,W1,...]] [--scan-below T] [--scan-null R[,seed]] [--band-ess [L]] [--loo-pit]\n"
                    "                         [--loo-window W[,first]] [--modes [q1,q2,...]] [--modes-ess [L]] [--modes-corr]\n"
                    "                         [--modes-rank [L]] [--modes-indices] [--modes-hist [N]] [--modes-hpd m1[,m2,...]]\n"
                    "                         [--modes-pairs c1:c2[,c3:c4,...] [N]]\n"
                    "     [1] The directory of config_default.cfg, errors_default.cfg and the *_ctrl.list files (Config/default)\n"
                    "     [2] The .model file and [3] the .data file of the fit\n"
                    "     [4] The root of the parameter files: <root>_chain-<m>.bin and <root>.hdr\n"
                    "     [5] The output file (ASCII): x y mean_M sd_M min_M max_M lppd var_l [one column per quantile] [elpd_loo pareto_k]\n"
                    "         [pit log_cdf log_sf mean_resid]\n"
                    "     --chain m   chain to read (default 0, the coldest)     --slice s   slice of the .model file, from 0 (default 0)\n"
                    "     --first i / --last j / --thin k   samples i, i + k, ... <= j, counted from 0 (default: all)\n"
                    "     --block B   samples per block on the GPU (default 0: chosen by the library)\n"
                    "     --quantiles q1,q2,...   up to 8 values in [0, 1]: one more column each, the exact quantile of the model per bin\n"
                    "                             (the samples are read again once per pass)     --qbits b   bits per pass, 1 ... 6 (default 0: the library's)\n"
                    "     --loo   PSIS-LOO: two more columns, elpd_loo and the Pareto k-hat per bin, and their totals in the header\n"
                    "             (the samples are read once more)\n"
                    "     --predictive   posterior predictive check: four last columns, pit, log_cdf, log_sf and mean_resid per bin, and\n"
                    "             two header lines with the totals and the PIT histogram (no further pass)\n"
                    "     --window W[,first]   the same check over disjoint windows of W bins (1 ... 512; likelihood p times W at most 512),\n"
                    "             the first window `first` bins long (1 ... W, default W): written to <output file>.windows, one row per\n"
                    "             window, w first_bin last_bin x_first x_last pit log_cdf log_sf mean_resid (no further pass; [5] is unchanged)\n"
                    "     --scan W0[,W1,...]   that check at every start position of up to 8 strictly ascending widths (each 1 ... 512 and at\n"
                    "             most the number of bins; likelihood p times the largest at most 512): written to <output file>.scan, one\n"
                    "             row per bin j, j x_j and per width pit log_cdf log_sf mean_resid, and the runs of positions below the line to\n"
                    "             <output file>.scan.regions, W which pos_first pos_last bin_first bin_last x_first x_last pos_min min_log\n"
                    "             mean_resid_at_min (no further pass; [5] and .windows are unchanged)\n"
                    "     --scan-below T   the line of the regions for all widths, T < 0 (default: log(0.01 W / Nx) per width)\n"
                    "     --scan-null R[,seed]   needs --scan: R >= 99 replicate noise spectra simulated on the device (seed default 0) give the\n"
                    "             joint 1 %% line over all positions and widths, the regions' line unless --scan-below is given, one more header\n"
                    "             line in .scan.regions, `# null= R seed alpha= 0.01 joint_line= ...`, and two trailing columns p_width p_joint\n"
                    "     --ess [L]   effective sample size, Monte-Carlo standard error and split R-hat per bin from the autocorrelation up\n"
                    "             to lag L (0 ... 1023, default 0: the library's 255): written to <output file>.ess, one row per bin,\n"
                    "             x ess_M tau_M mcse_M rhat_M cut_M ess_l r_eff cut_l (the samples are read once more; [5] is unchanged)\n"
                    "     --band-ess [L]   needs --quantiles: the effective sample size of every quantile, that of the indicator model <= quantile,\n"
                    "             from its autocorrelation up to lag L (0 ... 1023, default 0: the library's 255): written to <output file>.bandess,\n"
                    "             one row per bin, x and per quantile value count_le p_hat ess tau mcse_p cut (the samples are read once more\n"
                    "             after the selection; [5] is unchanged)\n"
                    "     --loo-pit   implies --loo: the leave-one-out PIT, the predictive tails under the PSIS weights, and the weights'\n"
                    "             effective sample size: written to <output file>.loopit, one row per bin,\n"
                    "             x loo_pit loo_log_cdf loo_log_sf is_ess pareto_k (the samples are read a third time)\n"
                    "     --loo-window W[,first]   leave-one-window-out PSIS-LOO over disjoint windows of W bins (1 ... 512), the first window\n"
                    "             `first` bins long (1 ... W, default W): written to <output file>.loowin, one row per window,\n"
                    "             first_bin last_bin x_first x_last elpd_lwo pareto_k tail_len, and with --loo-pit (likelihood p times W at\n"
                    "             most 512) loo_pit loo_log_cdf loo_log_sf is_ess log_wsum as well (the samples are read once more, with\n"
                    "             --loo-pit twice; [5] and the other files are unchanged)\n"
                    "     --modes [q1,q2,...]   the posterior mode table: per derived quantity of every multiplet and of the chain (frequency,\n"
                    "             width, height, amplitude, splitting, truncation window, component frequencies and heights; inclination,\n"
                    "             eta, a3, asymmetry) its mean, sd, min, max and exact quantiles (up to 8 values in [0, 1], default\n"
                    "             0.16,0.5,0.84) over the samples the summary used: written to <output file>.modes, one row per quantity,\n"
                    "             col kind mult order l m param_index mean sd min max and one column per quantile, 17 significant digits\n"
                    "             (the samples are read once more; [5] and the other files are unchanged)\n"
                    "     --modes-ess [L]   needs --modes: effective sample size, Monte-Carlo standard error and split R-hat of every quantity of\n"
                    "             the mode table from its autocorrelation up to lag L (0 ... 1023, default 0: the library's 255): written to\n"
                    "             <output file>.modes.ess, one row per quantity, col kind mult order l m param_index ess tau mcse rhat cut\n"
                    "     --modes-corr   needs --modes: the correlation matrix of the chain-level quantities and of freq width height amplitude\n"
                    "             splitting of every multiplet (at most 1024 columns): written to <output file>.modes.corr, `# cols = ...` and\n"
                    "             one matrix row per line (neither option reads the samples again; [5] and .modes are unchanged)\n"
                    "     --modes-rank [L]   needs --modes: rank-normalised diagnostics of every quantity of the mode table (bulk and tail\n"
                    "             effective sample size, rank-normalised and folded split R-hat; lag limit L as for --modes-ess): written to\n"
                    "             <output file>.modes.rank, one row per quantity, col kind mult order l m param_index ess_bulk ess_tail rhat\n"
                    "             tau_bulk rhat_bulk rhat_fold ess_q05 ess_q95 cut_z cut_zfold cut_i05 cut_i95\n"
                    "     --modes-indices   needs --modes: the seismic indices per sample (Dnu and epsilon of the radial ridge, nu_max,\n"
                    "             separations, second differences, d02 d13 d01 d10, r02 r01 r13 r10), reference row = the first accepted\n"
                    "             sample: written to <output file>.modes.indices, one row per index, col kind l n mean sd, one column per\n"
                    "             quantile of --modes, and the columns of --modes-ess / --modes-rank where given; the covariance matrix of\n"
                    "             the ratios to <output file>.modes.indices.cov (the samples are read once more; the other files are unchanged)\n"
                    "     --modes-hist [N]   needs --modes: the marginal histogram of every quantity of the mode table in N uniform classes\n"
                    "             (1 ... 4096, default 50) over its min ... max: written to <output file>.modes.hist, one block per quantity,\n"
                    "             range, below / above, then edge and count per class\n"
                    "     --modes-hpd m1[,m2,...]   needs --modes: the shortest interval holding each mass (up to 8 values in (0, 1]) of every\n"
                    "             quantity of the mode table: written to <output file>.modes.hpd, one row per quantity, col kind mult order l m\n"
                    "             param_index median and per mass k lo hi\n"
                    "     --modes-pairs c1:c2[,c3:c4,...] [N]   needs --modes: the joint histogram of each pair of table columns in N x N classes\n"
                    "             (1 ... 128, default 32) with its 68 %% and 95 %% contour levels: written to <output file>.modes.pairs (none of\n"
                    "             the three reads the samples again; the other files are unchanged)\n"
                    " chainsummary_hip version   prints the library version\n");
    return EXIT_FAILURE;
}

static int fail(const std::string &msg)
{
    fprintf(stderr, "chainsummary_hip: %s\n", msg.c_str());
    return EXIT_FAILURE;
}

// `! Nvars= 12` of a .hdr file; -1 when the key is missing
static long header_value(const std::string &hdr, const std::string &key)
{
    std::ifstream f(hdr.c_str());
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] != '!') continue;
        const size_t eq = line.find('=');
        if (eq == std::string::npos) continue;
        std::string k = line.substr(1, eq - 1);
        const size_t b = k.find_first_not_of(" \t");
        if (b == std::string::npos) continue;
        k = k.substr(b, k.find_last_not_of(" \t") - b + 1);
        if (k == key) return strtol(line.c_str() + eq + 1, nullptr, 10);
    }
    return -1;
}

int main(int argc, char *argv[])
{
    if (argc == 2 && std::string(argv[1]) == "version") { printf("chainsummary_hip (%s)\n", tamcmc_version()); return 0; }
    if (argc < 6) return usage();
    const std::string cfg_dir = argv[1], model_file = argv[2], data_file = argv[3], root = argv[4], out_file = argv[5];
    long chain = 0, slice = 0, first = 0, last = -1, thin = 1, block = 0, qbits = 0;
    std::vector<double> quant;
    std::string quant_text;
    bool loo = false, loo_pit = false, predictive = false;
    long win_W = 0, win_first = 0, ess_lag = -1;            // ess_lag < 0: no --ess
    long band_lag = -1;                                     // < 0: no --band-ess
    long lw_W = 0, lw_first = 0;                            // lw_W = 0: no --loo-window
    bool modes = false;                                     // --modes
    long modes_ess_lag = -1;                                // < 0: no --modes-ess
    bool modes_corr = false;                                // --modes-corr
    long modes_rank_lag = -1;                               // < 0: no --modes-rank
    bool modes_indices = false;                             // --modes-indices
    long hist_bins = 0;                                     // 0: no --modes-hist
    std::vector<double> hpd_mass;                           // empty: no --modes-hpd
    std::string hpd_text;
    std::vector<int32_t> pair_cols;                         // empty: no --modes-pairs
    long pair_bins = 32;
    std::vector<double> mquant;
    std::string mquant_text = "0.16,0.5,0.84";
    std::vector<int32_t> scan_W;
    std::string scan_text;
    double scan_below = std::nan("");                       // NaN: the library's default line per width
    bool have_below = false;
    long long null_R = 0;                                   // 0: no --scan-null
    unsigned long long null_seed = 0;
    const double null_alpha = 0.01;
    for (int i = 6; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--loo") { loo = true; continue; }
        if (a == "--loo-pit") { loo = loo_pit = true; continue; }
        if (a == "--predictive") { predictive = true; continue; }
        if (a == "--ess") {                         // alone, or followed by the lag limit
            if (ess_lag >= 0) return usage();
            ess_lag = 0;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {
                char *end = nullptr;
                ess_lag = strtol(argv[++i], &end, 10);
                if (*end != '\0' || ess_lag > TAMCMC_SUMMARY_ESS_MAX_LAG) return usage();
            }
            continue;
        }
        if (a == "--modes") {                       // alone, or followed by the list of quantiles
            if (modes) return usage();
            modes = true;
            if (i + 1 < argc && ((argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') || argv[i + 1][0] == '.')) mquant_text = argv[++i];
            for (const char *p = mquant_text.c_str();;) {
                char *end = nullptr;
                const double q = strtod(p, &end);
                if (end == p || !(q >= 0.0 && q <= 1.0) || mquant.size() >= TAMCMC_SUMMARY_MAX_QUANTILES) return usage();
                mquant.push_back(q);
                if (*end == '\0') break;
                if (*end != ',') return usage();
                p = end + 1;
            }
            continue;
        }
        if (a == "--modes-ess") {                   // alone, or followed by the lag limit
            if (modes_ess_lag >= 0) return usage();
            modes_ess_lag = 0;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {
                char *end = nullptr;
                modes_ess_lag = strtol(argv[++i], &end, 10);
                if (*end != '\0' || modes_ess_lag > TAMCMC_MODEDIAG_MAX_LAG) return usage();
            }
            continue;
        }
        if (a == "--modes-rank") {                  // alone, or followed by the lag limit
            if (modes_rank_lag >= 0) return usage();
            modes_rank_lag = 0;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {
                char *end = nullptr;
                modes_rank_lag = strtol(argv[++i], &end, 10);
                if (*end != '\0' || modes_rank_lag > TAMCMC_MODEDIAG_MAX_LAG) return usage();
            }
            continue;
        }
        if (a == "--modes-corr") {
            if (modes_corr) return usage();
            modes_corr = true;
            continue;
        }
        if (a == "--modes-indices") {
            if (modes_indices) return usage();
            modes_indices = true;
            continue;
        }
        if (a == "--modes-hist") {                  // alone, or followed by the number of classes
            if (hist_bins != 0) return usage();
            hist_bins = 50;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {
                char *end = nullptr;
                hist_bins = strtol(argv[++i], &end, 10);
                if (*end != '\0' || hist_bins < 1 || hist_bins > TAMCMC_MODEPDF_MAX_BINS) return usage();
            }
            continue;
        }
        if (a == "--modes-hpd") {
            if (i + 1 >= argc || !hpd_mass.empty()) return usage();
            hpd_text = argv[++i];
            for (const char *p = hpd_text.c_str();;) {
                char *end = nullptr;
                const double m = strtod(p, &end);
                if (end == p || !(m > 0.0 && m <= 1.0) || hpd_mass.size() >= TAMCMC_MODEPDF_MAX_MASS) return usage();
                hpd_mass.push_back(m);
                if (*end == '\0') break;
                if (*end != ',') return usage();
                p = end + 1;
            }
            continue;
        }
        if (a == "--modes-pairs") {                 // the pairs, then alone or followed by the number of classes an axis
            if (i + 1 >= argc || !pair_cols.empty()) return usage();
            for (const char *p = argv[++i];;) {
                char *end = nullptr;
                if (*p < '0' || *p > '9') return usage();
                const long c1 = strtol(p, &end, 10);
                if (*end != ':' || end[1] < '0' || end[1] > '9') return usage();
                p = end + 1;
                const long c2 = strtol(p, &end, 10);
                if (c1 > 0x7FFFFFFF || c2 > 0x7FFFFFFF || pair_cols.size() >= 2 * (size_t)TAMCMC_MODEPDF_MAX_PAIRS) return usage();
                pair_cols.push_back((int32_t)c1); pair_cols.push_back((int32_t)c2);
                if (*end == '\0') break;
                if (*end != ',') return usage();
                p = end + 1;
            }
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {
                char *end = nullptr;
                pair_bins = strtol(argv[++i], &end, 10);
                if (*end != '\0' || pair_bins < 1 || pair_bins > TAMCMC_MODEPDF_MAX_BINS2D) return usage();
            }
            continue;
        }
        if (a == "--band-ess") {                    // alone, or followed by the lag limit
            if (band_lag >= 0) return usage();
            band_lag = 0;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {
                char *end = nullptr;
                band_lag = strtol(argv[++i], &end, 10);
                if (*end != '\0' || band_lag > TAMCMC_SUMMARY_ESS_MAX_LAG) return usage();
            }
            continue;
        }
        if (a == "--window") {                      // W or W,first
            if (i + 1 >= argc || win_W != 0) return usage();
            char *end = nullptr;
            const char *p = argv[++i];
            win_W = strtol(p, &end, 10);
            if (end == p || win_W < 1 || win_W > TAMCMC_SUMMARY_WINDOW_MAX_BINS) return usage();
            win_first = win_W;
            if (*end == ',') {
                p = end + 1;
                win_first = strtol(p, &end, 10);
                if (end == p || win_first < 1 || win_first > win_W) return usage();
            }
            if (*end != '\0') return usage();
            continue;
        }
        if (a == "--loo-window") {                  // W or W,first
            if (i + 1 >= argc || lw_W != 0) return usage();
            const char *p = argv[++i];
            char *end = nullptr;
            lw_W = strtol(p, &end, 10);
            if (end == p || lw_W < 1 || lw_W > TAMCMC_SUMMARY_WINDOW_MAX_BINS) return usage();
            if (*end == ',') {
                p = end + 1;
                lw_first = strtol(p, &end, 10);
                if (end == p || lw_first < 1 || lw_first > lw_W) return usage();
            }
            if (*end != '\0') return usage();
            continue;
        }
        if (a == "--scan") {                        // a comma-separated, strictly ascending list of widths
            if (i + 1 >= argc || !scan_W.empty()) return usage();
            scan_text = argv[++i];
            for (const char *p = scan_text.c_str();;) {
                char *end = nullptr;
                const long W = strtol(p, &end, 10);
                if (end == p || W < 1 || W > TAMCMC_SUMMARY_WINDOW_MAX_BINS || scan_W.size() >= TAMCMC_SUMMARY_SCAN_MAX_WIDTHS ||
                    (!scan_W.empty() && W <= scan_W.back()))
                    return usage();
                scan_W.push_back((int32_t)W);
                if (*end == '\0') break;
                if (*end != ',') return usage();
                p = end + 1;
            }
            continue;
        }
        if (a == "--scan-below") {                  // a negative number
            if (i + 1 >= argc || have_below) return usage();
            char *end = nullptr;
            const char *p = argv[++i];
            scan_below = strtod(p, &end);
            if (end == p || *end != '\0' || !(scan_below < 0.0)) return usage();
            have_below = true;
            continue;
        }
        if (a == "--scan-null") {                   // R or R,seed
            if (i + 1 >= argc || null_R != 0) return usage();
            char *end = nullptr;
            const char *p = argv[++i];
            if (*p < '0' || *p > '9') return usage();
            null_R = strtoll(p, &end, 10);
            if (end == p || null_R > TAMCMC_SCAN_NULL_MAX_REPLICATES || std::floor(null_alpha * (double)(null_R + 1)) < 1.0) return usage();
            if (*end == ',') {
                p = end + 1;
                if (*p < '0' || *p > '9') return usage();
                null_seed = strtoull(p, &end, 10);
            }
            if (*end != '\0') return usage();
            continue;
        }
        if (a == "--quantiles") {                   // a comma-separated list of numbers in [0, 1]
            if (i + 1 >= argc || !quant.empty()) return usage();
            quant_text = argv[++i];
            for (const char *p = quant_text.c_str();;) {
                char *end = nullptr;
                const double q = strtod(p, &end);
                if (end == p || !(q >= 0.0 && q <= 1.0) || quant.size() >= TAMCMC_SUMMARY_MAX_QUANTILES) return usage();
                quant.push_back(q);
                if (*end == '\0') break;
                if (*end != ',') return usage();
                p = end + 1;
            }
            continue;
        }
        long *dst = a == "--qbits" ? &qbits : a == "--chain" ? &chain : a == "--slice" ? &slice : a == "--first" ? &first : a == "--last" ? &last :
                    a == "--thin" ? &thin : a == "--block" ? &block : nullptr;
        char *end = nullptr;
        if (!dst || i + 1 >= argc) return usage();
        *dst = strtol(argv[++i], &end, 10);
        if (end == argv[i] || *end != '\0') return usage();
    }
    if (chain < 0 || slice < 0 || first < 0 || thin < 1 || block < 0 || block > 0x7FFFFFFF || qbits < 0 || qbits > 6) return usage();
    if ((have_below || null_R) && scan_W.empty()) return usage();
    if ((modes_ess_lag >= 0 || modes_corr) && !modes) { fprintf(stderr, "chainsummary_hip: --modes-ess and --modes-corr need --modes\n"); return usage(); }
    if (modes_rank_lag >= 0 && !modes) { fprintf(stderr, "chainsummary_hip: --modes-rank needs --modes\n"); return usage(); }
    if (modes_indices && !modes) { fprintf(stderr, "chainsummary_hip: --modes-indices needs --modes\n"); return usage(); }
    if ((hist_bins != 0 || !hpd_mass.empty() || !pair_cols.empty()) && !modes) {
        fprintf(stderr, "chainsummary_hip: --modes-hist, --modes-hpd and --modes-pairs need --modes\n");
        return usage();
    }
    if (band_lag >= 0 && quant.empty()) { fprintf(stderr, "chainsummary_hip: --band-ess needs --quantiles\n"); return usage(); }

    tamcmc_setup *S = nullptr;
    if (tamcmc_setup_create(&S, cfg_dir.c_str()) != TAMCMC_IO_OK) return fail("cannot read the default configuration in " + cfg_dir);
    if (tamcmc_setup_load(S, model_file.c_str(), data_file.c_str(), (int32_t)slice) != TAMCMC_IO_OK)
        return fail("reading " + model_file + " / " + data_file + ": " + tamcmc_setup_error(S));
    int32_t Nparams = 0, Nvars = 0, plength[11], model_case = 0, like_case = 0, prior_case = 0;
    int64_t Nx = 0;
    double like_p = 1.0;
    tamcmc_setup_sizes(S, &Nparams, &Nvars, &Nx, plength, &model_case, &like_case, &prior_case, &like_p);
    std::vector<double> x(Nx), y(Nx), sig(Nx), inputs(Nparams);
    std::vector<int32_t> relax(Nparams), idx;
    tamcmc_setup_data(S, x.data(), y.data(), sig.data());
    tamcmc_setup_inputs(S, inputs.data(), relax.data(), nullptr, nullptr, nullptr, nullptr);
    tamcmc_setup_destroy(S);
    for (int32_t i = 0; i < Nparams; i++) if (relax[i] == 1) idx.push_back(i);      // Model_def::index_to_relax, model_def.cpp:81-88
    if ((int32_t)idx.size() != Nvars) return fail("the setup's relax mask does not match its Nvars");

    const long hv = header_value(root + ".hdr", "Nvars");
    if (hv < 0) return fail("cannot read Nvars from " + root + ".hdr");
    if (hv != Nvars) return fail("Nvars = " + std::to_string(hv) + " in " + root + ".hdr, but the setup has " + std::to_string(Nvars) + " variables");
    const std::string bin = root + "_chain-" + std::to_string(chain) + ".bin";
    std::ifstream f(bin.c_str(), std::ios::binary);
    if (!f.is_open()) return fail("unable to open " + bin);
    f.seekg(0, std::ios::end);
    const long long fbytes = (long long)f.tellg();
    f.seekg(0, std::ios::beg);
    const long long rowb = (long long)Nvars * (long long)sizeof(double);
    if (Nvars < 1 || fbytes < rowb || fbytes % rowb != 0) return fail(bin + " does not hold whole rows of " + std::to_string(Nvars) + " doubles");
    const long long Nrows = fbytes / rowb;
    if (last < 0 || last >= Nrows) last = (long)(Nrows - 1);
    if (first > last) return fail("no sample in the requested range (the file has " + std::to_string(Nrows) + ")");
    const long long Nsel = (last - first) / thin + 1;

    tamcmc_ctx *ctx = nullptr;
    int rc = tamcmc_ctx_create(&ctx, 0, model_case, like_case, like_p, plength, Nx, x.data(), y.data(), sig.data());
    if (rc != TAMCMC_OK) return fail(std::string("tamcmc_ctx_create: ") + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error());
    tamcmc_summary *sum = nullptr;
    rc = tamcmc_summary_create(&sum, ctx, (int32_t)block);
    if (rc != TAMCMC_OK) return fail(std::string("tamcmc_summary_create: ") + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error());
    if (predictive) {
        rc = tamcmc_summary_predictive_enable(sum);
        if (rc != TAMCMC_OK) return fail(std::string("tamcmc_summary_predictive_enable: ") + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error());
    }
    int32_t n_windows = 0;
    if (win_W) {
        rc = tamcmc_summary_window_enable(sum, (int32_t)win_W, (int32_t)win_first, &n_windows);
        if (rc != TAMCMC_OK) return fail(std::string("tamcmc_summary_window_enable: ") + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error());
    }
    if (!scan_W.empty()) {
        rc = tamcmc_summary_scan_enable(sum, (int32_t)scan_W.size(), scan_W.data());
        if (rc != TAMCMC_OK) return fail(std::string("tamcmc_summary_scan_enable: ") + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error());
    }
    // One pass over the selected samples, a few thousand rows per push: the library cuts them into its blocks.
    const long long chunk = 4096;
    std::vector<double> vars((size_t)Nvars), P;
    long long last_used = first;
    // --modes: the status of every selected sample in the fold pass (what the fold skipped the mode table skips), and,
    // while mt_push is set, the pass that feeds the mode table instead of the summary
    std::vector<int32_t> fold_status(modes ? (size_t)Nsel : 0), mt_skip;
    bool fold_pass = true;
    tamcmc_modetable *mt_push = nullptr;
    // the params row of sample `at` of the file: the model's inputs with the stored variables put in
    auto read_row = [&](long long at, double *row) -> bool {
        f.seekg(at * rowb, std::ios::beg);
        f.read(reinterpret_cast<char *>(vars.data()), (std::streamsize)rowb);
        if (!f) return false;
        std::memcpy(row, inputs.data(), (size_t)Nparams * sizeof(double));
        for (int32_t v = 0; v < Nvars; v++) row[idx[(size_t)v]] = vars[(size_t)v];
        return true;
    };
    auto push_selected = [&]() -> int {
        for (long long k0 = 0; k0 < Nsel; k0 += chunk) {
            const long long n = Nsel - k0 < chunk ? Nsel - k0 : chunk;
            P.assign((size_t)n * (size_t)Nparams, 0.0);
            for (long long k = 0; k < n; k++) {
                last_used = first + (k0 + k) * thin;
                if (!read_row(last_used, P.data() + (size_t)k * (size_t)Nparams)) return fail("short read in " + bin);
            }
            if (mt_push) {
                mt_skip.assign(fold_status.begin() + k0, fold_status.begin() + k0 + n);
                rc = tamcmc_modetable_push(mt_push, (int32_t)n, Nparams, P.data(), mt_skip.data(), nullptr);
                if (rc != TAMCMC_OK) return fail(std::string("tamcmc_modetable_push: ") + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error());
                continue;
            }
            rc = tamcmc_summary_push(sum, (int32_t)n, Nparams, P.data(), nullptr, modes && fold_pass ? fold_status.data() + k0 : nullptr);
            if (rc != TAMCMC_OK) return fail(std::string("tamcmc_summary_push: ") + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error());
        }
        return 0;
    };
    if (push_selected() != 0) return EXIT_FAILURE;
    fold_pass = false;
    // --modes-indices: the reference row of the indices, the first selected sample that the fold took and whose derivation the
    // mode table accepts.  The samples the fold took are derived one at a time until one is accepted: usually the first.
    std::vector<double> ref_row;
    auto find_reference = [&](tamcmc_modetable *probe, int32_t n_cols) -> int {
        std::vector<double> row((size_t)Nparams), derived((size_t)n_cols);
        for (long long k = 0; k < Nsel; k++) {
            if (fold_status[(size_t)k] != TAMCMC_CHAIN_OK) continue;
            if (!read_row(first + k * thin, row.data())) return fail("short read in " + bin);
            int32_t st = -1;
            rc = tamcmc_modetable_derive(probe, 1, Nparams, row.data(), derived.data(), &st);
            if (rc != TAMCMC_OK) return fail(std::string("tamcmc_modetable_derive: ") + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error());
            if (st == TAMCMC_CHAIN_OK) { ref_row = row; break; }
        }
        return 0;
    };
    tamcmc_summary_totals t;
    std::vector<double> mean_M(Nx), var_M(Nx), min_M(Nx), max_M(Nx), var_l(Nx), lppd(Nx);
    rc = tamcmc_summary_result(sum, &t, mean_M.data(), var_M.data(), min_M.data(), max_M.data(), nullptr, var_l.data(), lppd.data());
    if (rc != TAMCMC_OK) return fail(std::string("tamcmc_summary_result: ") + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error());
    tamcmc_summary_predictive_totals pt{};
    const size_t Np = predictive ? (size_t)Nx : 0;
    std::vector<double> pit(Np), log_cdf(Np), log_sf(Np), mean_resid(Np);
    if (predictive) {
        rc = tamcmc_summary_predictive_result(sum, &pt, pit.data(), log_cdf.data(), log_sf.data(), mean_resid.data());
        if (rc != TAMCMC_OK) return fail(std::string("tamcmc_summary_predictive_result: ") + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error());
    }
    tamcmc_summary_window_totals wt{};
    std::vector<double> wpit((size_t)n_windows), wlog_cdf((size_t)n_windows), wlog_sf((size_t)n_windows), wmean_resid((size_t)n_windows);
    if (win_W) {
        rc = tamcmc_summary_window_result(sum, &wt, wpit.data(), wlog_cdf.data(), wlog_sf.data(), wmean_resid.data());
        if (rc != TAMCMC_OK) return fail(std::string("tamcmc_summary_window_result: ") + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error());
    }
    // the scan: per width the four arrays over its positions and the regions of either side
    const size_t Ks = scan_W.size();
    std::vector<tamcmc_summary_scan_totals> st(Ks);
    std::vector<std::vector<double>> sarr(4 * Ks);              // width k: pit, log_cdf, log_sf, mean_resid at 4 k ... 4 k + 3
    std::vector<std::vector<tamcmc_summary_scan_region>> sreg(2 * Ks);      // width k, side `which` at 2 k + which
    // the null of the scan: the joint line of width k, side `which` at 2 k + which, and the two p-values of every region
    std::vector<double> joint_line(2 * Ks, std::nan(""));
    std::vector<std::vector<double>> sreg_p(2 * Ks);           // p_width, p_joint of region i at 2 i, 2 i + 1
    tamcmc_scan_null *null = nullptr;
    if (null_R) {
        rc = tamcmc_scan_null_create(&null, 0, like_case, like_p, Nx, (int32_t)Ks, scan_W.data(), null_seed, 0);
        if (rc == TAMCMC_OK) rc = tamcmc_scan_null_run(null, null_R);
        for (size_t i = 0; i < 2 * Ks && rc == TAMCMC_OK; i++) rc = tamcmc_scan_null_line(null, (int32_t)(i / 2), (int32_t)(i % 2), null_alpha, 1, &joint_line[i]);
        if (rc != TAMCMC_OK) return fail(std::string("tamcmc_scan_null: ") + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error());
    }
    for (size_t k = 0; k < Ks; k++) {
        auto sfail = [&](const char *what) { return fail(std::string(what) + ": " + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error()); };
        const size_t n_pos = (size_t)(Nx - scan_W[k] + 1);
        for (int c = 0; c < 4; c++) sarr[4 * k + c].resize(n_pos);
        rc = tamcmc_summary_scan_result(sum, (int32_t)k, &st[k], sarr[4 * k].data(), sarr[4 * k + 1].data(), sarr[4 * k + 2].data(), sarr[4 * k + 3].data());
        if (rc != TAMCMC_OK) return sfail("tamcmc_summary_scan_result");
        for (int which = 0; which < 2; which++) {
            int32_t n_reg = 0;
            const double line = null_R && !have_below ? joint_line[2 * k + (size_t)which] : scan_below;
            rc = tamcmc_summary_scan_regions(sum, (int32_t)k, which, line, 0, nullptr, &n_reg);
            if (rc != TAMCMC_OK) return sfail("tamcmc_summary_scan_regions");
            std::vector<tamcmc_summary_scan_region> &r = sreg[2 * k + (size_t)which];
            r.resize((size_t)n_reg);
            if (n_reg > 0) rc = tamcmc_summary_scan_regions(sum, (int32_t)k, which, line, n_reg, r.data(), &n_reg);
            if (rc != TAMCMC_OK) return sfail("tamcmc_summary_scan_regions");
            std::vector<double> &pv = sreg_p[2 * k + (size_t)which];
            pv.resize(null_R ? 2 * r.size() : 0);
            for (size_t i = 0; null_R && i < r.size(); i++) {
                rc = tamcmc_scan_null_pvalue(null, (int32_t)k, which, r[i].min_log, &pv[2 * i], &pv[2 * i + 1]);
                if (rc != TAMCMC_OK) return sfail("tamcmc_scan_null_pvalue");
            }
        }
    }
    tamcmc_scan_null_destroy(null);
    // quantiles: the same samples again, once per pass, until every value is exact
    const size_t Nq = quant.size();
    std::vector<double> qlo(Nq * (size_t)Nx);
    int passes = 0;
    if (Nq) {
        auto qfail = [&](const char *what) { return fail(std::string(what) + ": " + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error()); };
        rc = tamcmc_summary_quantiles_begin(sum, (int32_t)Nq, quant.data(), (int32_t)qbits);
        if (rc != TAMCMC_OK) return qfail("tamcmc_summary_quantiles_begin");
        for (int32_t left = 1; left > 0; passes++) {              // (a chain whose samples are all equal takes one idle pass)
            if (push_selected() != 0) return EXIT_FAILURE;
            rc = tamcmc_summary_quantiles_step(sum, &left);
            if (rc != TAMCMC_OK) return qfail("tamcmc_summary_quantiles_step");
        }
        rc = tamcmc_summary_quantiles_result(sum, nullptr, qlo.data(), nullptr);
        if (rc != TAMCMC_OK) return qfail("tamcmc_summary_quantiles_result");
        tamcmc_summary_quantiles_end(sum);
    }
    // band ESS: the same samples once more, in the same order, against the exact quantiles
    tamcmc_summary_bandess_totals bt{};
    const size_t Nb = band_lag >= 0 ? Nq * (size_t)Nx : 0;
    std::vector<double> b_p(Nb), b_ess(Nb), b_tau(Nb), b_mcse(Nb);
    std::vector<int32_t> b_count(Nb), b_cut(Nb);
    if (band_lag >= 0) {
        auto bfail = [&](const char *what) { return fail(std::string(what) + ": " + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error()); };
        rc = tamcmc_summary_bandess_begin(sum, (int32_t)Nq, qlo.data(), (int32_t)band_lag, nullptr);
        if (rc != TAMCMC_OK) return bfail("tamcmc_summary_bandess_begin");
        if (push_selected() != 0) return EXIT_FAILURE;
        rc = tamcmc_summary_bandess_result(sum, &bt, b_count.data(), b_p.data(), b_ess.data(), b_tau.data(), b_mcse.data(), b_cut.data());
        if (rc != TAMCMC_OK) return bfail("tamcmc_summary_bandess_result");
        tamcmc_summary_bandess_end(sum);
    }
    // PSIS-LOO: the same samples once more
    tamcmc_summary_loo_totals lt{};
    std::vector<double> elpd(loo ? (size_t)Nx : 0), khat(loo ? (size_t)Nx : 0);
    tamcmc_summary_loo_pit_totals lpt{};
    const size_t Nlp = loo_pit ? (size_t)Nx : 0;
    std::vector<double> lp_pit(Nlp), lp_cdf(Nlp), lp_sf(Nlp), lp_ess(Nlp);
    if (loo) {
        auto lfail = [&](const char *what) { return fail(std::string(what) + ": " + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error()); };
        rc = tamcmc_summary_loo_begin(sum);
        if (rc != TAMCMC_OK) return lfail("tamcmc_summary_loo_begin");
        if (push_selected() != 0) return EXIT_FAILURE;
        rc = tamcmc_summary_loo_result(sum, &lt, elpd.data(), khat.data(), nullptr, nullptr);
        if (rc != TAMCMC_OK) return lfail("tamcmc_summary_loo_result");
        if (loo_pit) {                                              // LOO-PIT: and a third time
            rc = tamcmc_summary_loo_pit_begin(sum);
            if (rc != TAMCMC_OK) return lfail("tamcmc_summary_loo_pit_begin");
            if (push_selected() != 0) return EXIT_FAILURE;
            rc = tamcmc_summary_loo_pit_result(sum, &lpt, lp_pit.data(), lp_cdf.data(), lp_sf.data(), lp_ess.data(), nullptr);
            if (rc != TAMCMC_OK) return lfail("tamcmc_summary_loo_pit_result");
        }
        tamcmc_summary_loo_end(sum);
    }
    // window-LOO: the same samples once more, and with --loo-pit a further time
    tamcmc_summary_wloo_totals lwt{};
    tamcmc_summary_loo_pit_totals lwpt{};
    std::vector<double> lw_elpd, lw_khat, lw_pit, lw_cdf, lw_sf, lw_ess, lw_wsum;
    std::vector<int32_t> lw_tail;
    std::vector<int64_t> lw_b, lw_e;
    if (lw_W) {
        auto wfail = [&](const char *what) { return fail(std::string(what) + ": " + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error()); };
        int32_t nw = 0;
        rc = tamcmc_summary_wloo_begin(sum, (int32_t)lw_W, (int32_t)lw_first, &nw);
        if (rc != TAMCMC_OK) return wfail("tamcmc_summary_wloo_begin");
        lw_elpd.resize((size_t)nw); lw_khat.resize((size_t)nw); lw_tail.resize((size_t)nw); lw_b.resize((size_t)nw); lw_e.resize((size_t)nw);
        if (push_selected() != 0) return EXIT_FAILURE;
        rc = tamcmc_summary_wloo_result(sum, &lwt, lw_elpd.data(), lw_khat.data(), nullptr, lw_tail.data(), lw_b.data(), lw_e.data());
        if (rc != TAMCMC_OK) return wfail("tamcmc_summary_wloo_result");
        if (loo_pit) {
            lw_pit.resize((size_t)nw); lw_cdf.resize((size_t)nw); lw_sf.resize((size_t)nw); lw_ess.resize((size_t)nw); lw_wsum.resize((size_t)nw);
            rc = tamcmc_summary_wloo_pit_begin(sum);
            if (rc != TAMCMC_OK) return wfail("tamcmc_summary_wloo_pit_begin");
            if (push_selected() != 0) return EXIT_FAILURE;
            rc = tamcmc_summary_wloo_pit_result(sum, &lwpt, lw_pit.data(), lw_cdf.data(), lw_sf.data(), lw_ess.data(), lw_wsum.data());
            if (rc != TAMCMC_OK) return wfail("tamcmc_summary_wloo_pit_result");
        }
        tamcmc_summary_wloo_end(sum);
    }
    // ESS, MCSE and split R-hat: the same samples once more, in the same order
    tamcmc_summary_ess_totals et{};
    const size_t Ne = ess_lag >= 0 ? (size_t)Nx : 0;
    std::vector<double> ess_M(Ne), tau_M(Ne), mcse_M(Ne), rhat_M(Ne), ess_l(Ne), r_eff(Ne);
    std::vector<int32_t> cut_M(Ne), cut_l(Ne);
    if (ess_lag >= 0) {
        auto efail = [&](const char *what) { return fail(std::string(what) + ": " + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error()); };
        rc = tamcmc_summary_ess_begin(sum, (int32_t)ess_lag, nullptr);
        if (rc != TAMCMC_OK) return efail("tamcmc_summary_ess_begin");
        if (push_selected() != 0) return EXIT_FAILURE;
        rc = tamcmc_summary_ess_result(sum, &et, ess_M.data(), tau_M.data(), mcse_M.data(), rhat_M.data(), cut_M.data(), ess_l.data(), r_eff.data(),
                                       cut_l.data());
        if (rc != TAMCMC_OK) return efail("tamcmc_summary_ess_result");
        tamcmc_summary_ess_end(sum);
    }
    tamcmc_summary_destroy(sum);
    // the mode table: the same samples once more; those the fold skipped are skipped
    tamcmc_modetable_totals mtt{};
    std::vector<tamcmc_modetable_col> m_col;
    std::vector<double> m_mean, m_sd, m_min, m_max, m_q;
    tamcmc_modediag_totals mdt{};                           // --modes-ess
    std::vector<double> d_ess, d_tau, d_mcse, d_rhat, d_corr;
    std::vector<int32_t> d_cut, head_cols;                  // --modes-corr: the headline columns
    tamcmc_moderank_totals mrt{};                           // --modes-rank
    std::vector<double> r_out;
    std::vector<int32_t> r_cut;
    std::vector<int64_t> h_cnt, h_below, h_above;           // --modes-hist
    std::vector<double> h_range;
    std::vector<int32_t> h_status;
    std::vector<int64_t> p_k, p_start;                      // --modes-hpd
    std::vector<double> p_lo, p_hi, p_med;
    std::vector<int64_t> j_cnt, j_out, j_level;             // --modes-pairs
    std::vector<double> j_range;
    std::vector<int32_t> j_status;
    tamcmc_seismic_info sinfo{};                            // --modes-indices
    tamcmc_modetable_totals stt{};
    std::vector<tamcmc_modetable_col> s_col;
    std::vector<double> s_mean, s_sd, s_q, s_ess, s_tau, s_mcse, s_rhat, s_rout, s_cov;
    std::vector<int32_t> s_cut, s_rcut, ratio_cols;
    if (modes) {
        auto mfail = [&](const char *what) { return fail(std::string(what) + ": " + tamcmc_strerror(rc) + " " + tamcmc_last_hip_error()); };
        tamcmc_modetable *mt = nullptr;
        rc = tamcmc_modetable_create(&mt, ctx, (int64_t)Nsel);
        if (rc != TAMCMC_OK) return mfail("tamcmc_modetable_create");
        int32_t n_cols = 0, n_mult = 0;
        tamcmc_modetable_columns(mt, &n_cols, &n_mult);
        const size_t nc = (size_t)n_cols;
        m_col.resize(nc); m_mean.resize(nc); m_sd.resize(nc); m_min.resize(nc); m_max.resize(nc);
        m_q.assign(mquant.size() * nc, std::nan(""));
        for (int32_t k = 0; k < n_cols; k++) tamcmc_modetable_column(mt, k, &m_col[(size_t)k]);
        if (modes_corr) {
            for (int32_t k = 0; k < n_cols; k++)
                if (m_col[(size_t)k].kind <= TAMCMC_MODETABLE_SPLITTING) head_cols.push_back(k);
            if (head_cols.size() > TAMCMC_MODEDIAG_MAX_COLS)
                return fail("--modes-corr: " + std::to_string(head_cols.size()) + " headline columns, more than " +
                            std::to_string(TAMCMC_MODEDIAG_MAX_COLS) + " of one correlation matrix");
        }
        mt_push = mt;
        if (push_selected() != 0) return EXIT_FAILURE;
        mt_push = nullptr;
        rc = tamcmc_modetable_result(mt, &mtt, m_mean.data(), m_sd.data(), m_min.data(), m_max.data());
        if (rc != TAMCMC_OK) return mfail("tamcmc_modetable_result");
        if (mtt.n_used > 0) {
            rc = tamcmc_modetable_quantiles(mt, (int32_t)mquant.size(), mquant.data(), nullptr, m_q.data());
            if (rc != TAMCMC_OK) return mfail("tamcmc_modetable_quantiles");
        }
        if (modes_ess_lag >= 0) {
            if (mtt.n_used < 4) return fail("--modes-ess needs at least 4 accepted samples");
            d_ess.resize(nc); d_tau.resize(nc); d_mcse.resize(nc); d_rhat.resize(nc); d_cut.resize(nc);
            rc = tamcmc_modediag_ess(mt, (int32_t)modes_ess_lag, &mdt, d_ess.data(), d_tau.data(), d_mcse.data(), d_rhat.data(), d_cut.data());
            if (rc != TAMCMC_OK) return mfail("tamcmc_modediag_ess");
        }
        if (modes_corr) {
            if (mtt.n_used < 2) return fail("--modes-corr needs at least 2 accepted samples");
            d_corr.resize(head_cols.size() * head_cols.size());
            rc = tamcmc_modediag_corr(mt, (int32_t)head_cols.size(), head_cols.data(), d_corr.data());
            if (rc != TAMCMC_OK) return mfail("tamcmc_modediag_corr");
        }
        if (modes_rank_lag >= 0) {
            if (mtt.n_used < 4) return fail("--modes-rank needs at least 4 accepted samples");
            r_out.resize((size_t)TAMCMC_MODERANK_NOUT * nc); r_cut.resize((size_t)TAMCMC_MODERANK_NSERIES * nc);
            rc = tamcmc_moderank_diag(mt, (int32_t)modes_rank_lag, n_cols, nullptr, 0, &mrt, r_out.data(), r_cut.data());
            if (rc != TAMCMC_OK) return mfail("tamcmc_moderank_diag");
        }
        if (hist_bins != 0) {
            if (mtt.n_used < 1) return fail("--modes-hist needs at least 1 accepted sample");
            h_cnt.resize(nc * (size_t)hist_bins); h_below.resize(nc); h_above.resize(nc); h_range.resize(2 * nc); h_status.resize(nc);
            rc = tamcmc_modepdf_hist(mt, (int32_t)hist_bins, n_cols, nullptr, nullptr, nullptr, h_cnt.data(), h_below.data(), h_above.data(),
                                     h_range.data(), h_status.data());
            if (rc != TAMCMC_OK) return mfail("tamcmc_modepdf_hist");
        }
        if (!hpd_mass.empty()) {
            if (mtt.n_used < 4) return fail("--modes-hpd needs at least 4 accepted samples");
            const size_t nm = hpd_mass.size();
            const double half = 0.5;
            p_k.resize(nm); p_start.resize(nm * nc); p_lo.resize(nm * nc); p_hi.resize(nm * nc); p_med.resize(nc);
            rc = tamcmc_modepdf_hpd(mt, (int32_t)nm, hpd_mass.data(), n_cols, nullptr, 0, p_k.data(), p_start.data(), p_lo.data(), p_hi.data());
            if (rc != TAMCMC_OK) return mfail("tamcmc_modepdf_hpd");
            rc = tamcmc_modetable_quantiles(mt, 1, &half, nullptr, p_med.data());
            if (rc != TAMCMC_OK) return mfail("tamcmc_modetable_quantiles");
        }
        if (!pair_cols.empty()) {
            if (mtt.n_used < 1) return fail("--modes-pairs needs at least 1 accepted sample");
            for (const int32_t c : pair_cols)
                if (c >= n_cols) return fail("--modes-pairs: column " + std::to_string(c) + " of a table of " + std::to_string(n_cols) + " columns");
            const size_t np = pair_cols.size() / 2, cells = (size_t)pair_bins * (size_t)pair_bins;
            const double levels[2] = {0.68, 0.95};
            j_cnt.resize(np * cells); j_out.resize(np); j_level.resize(2 * np); j_status.resize(np); j_range.resize(4 * np);
            rc = tamcmc_modepdf_hist2d(mt, (int32_t)pair_bins, (int32_t)np, pair_cols.data(), nullptr, nullptr, 2, levels, j_cnt.data(), j_out.data(),
                                       j_level.data(), j_status.data());
            if (rc != TAMCMC_OK) return mfail("tamcmc_modepdf_hist2d");
            for (size_t k = 0; k < 2 * np; k++) { j_range[2 * k] = m_min[(size_t)pair_cols[k]]; j_range[2 * k + 1] = m_max[(size_t)pair_cols[k]]; }
        }
        tamcmc_modetable_destroy(mt);
        mt = nullptr;
        // --modes-indices: a table of its own with the indices enabled, the same samples once more
        if (modes_indices) {
            rc = tamcmc_modetable_create(&mt, ctx, (int64_t)Nsel);
            if (rc != TAMCMC_OK) return mfail("tamcmc_modetable_create");
            if (find_reference(mt, n_cols) != 0) return EXIT_FAILURE;
            rc = ref_row.empty() ? TAMCMC_E_INVALID : tamcmc_modetable_indices_enable(mt, Nparams, ref_row.data(), &sinfo);
            if (rc == TAMCMC_E_INVALID) {
                fprintf(stderr, "chainsummary_hip: --modes-indices refused: %s; no .modes.indices file is written\n",
                        ref_row.empty() ? "no sample with an accepted derivation"
                                        : "the reference sample gives no plan (fewer than 3 radial modes, a radial order missing or the radial ridge "
                                          "not ascending, no index column, or a row too long for the kernel)");
                modes_indices = false;
            } else if (rc != TAMCMC_OK) return mfail("tamcmc_modetable_indices_enable");
        }
        if (modes_indices) {
            const size_t nb = (size_t)sinfo.n_base_cols, ni = (size_t)sinfo.n_index_cols, na = nb + ni;
            mt_push = mt;
            if (push_selected() != 0) return EXIT_FAILURE;
            mt_push = nullptr;
            s_col.resize(na); s_mean.resize(na); s_sd.resize(na); s_q.assign(mquant.size() * na, std::nan(""));
            for (size_t k = 0; k < na; k++) tamcmc_modetable_column(mt, (int32_t)k, &s_col[k]);
            rc = tamcmc_modetable_result(mt, &stt, s_mean.data(), s_sd.data(), nullptr, nullptr);
            if (rc != TAMCMC_OK) return mfail("tamcmc_modetable_result");
            const long long need = (modes_ess_lag >= 0 || modes_rank_lag >= 0) ? 4 : 2;
            if (stt.n_used < need) {
                fprintf(stderr, "chainsummary_hip: --modes-indices: %lld samples accepted with their indices, %lld needed; no .modes.indices file is written\n",
                        (long long)stt.n_used, need);
                modes_indices = false;
            }
        }
        if (modes_indices) {
            const size_t nb = (size_t)sinfo.n_base_cols, ni = (size_t)sinfo.n_index_cols, na = nb + ni;
            rc = tamcmc_modetable_quantiles(mt, (int32_t)mquant.size(), mquant.data(), nullptr, s_q.data());
            if (rc != TAMCMC_OK) return mfail("tamcmc_modetable_quantiles");
            if (modes_ess_lag >= 0) {
                tamcmc_modediag_totals unused{};
                s_ess.resize(na); s_tau.resize(na); s_mcse.resize(na); s_rhat.resize(na); s_cut.resize(na);
                rc = tamcmc_modediag_ess(mt, (int32_t)modes_ess_lag, &unused, s_ess.data(), s_tau.data(), s_mcse.data(), s_rhat.data(), s_cut.data());
                if (rc != TAMCMC_OK) return mfail("tamcmc_modediag_ess");
            }
            std::vector<int32_t> icols(ni);
            for (size_t k = 0; k < ni; k++) icols[k] = (int32_t)(nb + k);
            if (modes_rank_lag >= 0) {
                tamcmc_moderank_totals unused{};
                s_rout.resize((size_t)TAMCMC_MODERANK_NOUT * ni); s_rcut.resize((size_t)TAMCMC_MODERANK_NSERIES * ni);
                rc = tamcmc_moderank_diag(mt, (int32_t)modes_rank_lag, (int32_t)ni, icols.data(), 0, &unused, s_rout.data(), s_rcut.data());
                if (rc != TAMCMC_OK) return mfail("tamcmc_moderank_diag");
            }
            for (size_t k = nb; k < na; k++)
                if (s_col[k].kind >= TAMCMC_MODETABLE_R02 && s_col[k].kind <= TAMCMC_MODETABLE_R10) ratio_cols.push_back((int32_t)k);
            if (ratio_cols.size() > TAMCMC_MODEDIAG_MAX_COLS)
                return fail("--modes-indices: " + std::to_string(ratio_cols.size()) + " ratio columns, more than " +
                            std::to_string(TAMCMC_MODEDIAG_MAX_COLS) + " of one covariance matrix");
            s_cov.resize(ratio_cols.size() * ratio_cols.size());
            if (!ratio_cols.empty()) {
                rc = tamcmc_modediag_cov(mt, (int32_t)ratio_cols.size(), ratio_cols.data(), s_cov.data());
                if (rc != TAMCMC_OK) return mfail("tamcmc_modediag_cov");
            }
        }
        if (mt) tamcmc_modetable_destroy(mt);
    }
    tamcmc_ctx_destroy(ctx);

    FILE *o = fopen(out_file.c_str(), "w");
    if (!o) return fail("unable to open the output file " + out_file);
    fprintf(o, "# chainsummary_hip (%s)\n", tamcmc_version());
    fprintf(o, "# params= %s  chain= %ld  slice= %ld  model_case= %d  likelihood_case= %d\n", bin.c_str(), chain, slice, model_case, like_case);
    fprintf(o, "# samples_in_file= %lld  first= %ld  last= %lld  thin= %ld\n", Nrows, first, last_used, thin);
    fprintf(o, "# n_used= %lld  n_rejected= %lld\n", (long long)t.n_used, (long long)t.n_rejected);
    fprintf(o, "# lppd_total= %.12g  p_waic= %.12g  waic= %.12g\n", t.lppd_total, t.p_waic, t.waic);
    if (Nq) fprintf(o, "# quantiles= %s  passes= %d\n", quant_text.c_str(), passes);
    if (loo) fprintf(o, "# elpd_loo= %.12g  p_loo= %.12g  looic= %.12g  k_max= %.12g  n_k_high= %lld  n_k_inf= %lld\n", lt.elpd_loo, lt.p_loo, lt.looic,
                     lt.k_max, (long long)lt.n_k_high, (long long)lt.n_k_inf);
    if (predictive) {
        fprintf(o, "# ks_D= %.12g  min_log_sf= %.12g  bin_min_log_sf= %lld  min_log_cdf= %.12g  bin_min_log_cdf= %lld\n", pt.ks_D, pt.min_log_sf,
                (long long)pt.bin_min_log_sf, pt.min_log_cdf, (long long)pt.bin_min_log_cdf);
        fprintf(o, "# pit_hist=");
        for (int k = 0; k < TAMCMC_SUMMARY_PIT_CELLS; k++) fprintf(o, " %lld", (long long)pt.pit_hist[k]);
        fprintf(o, "\n");
    }
    fprintf(o, "# x y mean_M sd_M min_M max_M lppd var_l");
    for (size_t j = 0; j < Nq; j++) fprintf(o, " q%.6g", quant[j]);
    if (loo) fprintf(o, " elpd_loo pareto_k");
    if (predictive) fprintf(o, " pit log_cdf log_sf mean_resid");
    fprintf(o, "\n");
    for (int64_t i = 0; i < Nx; i++) {
        fprintf(o, "%.12g %.12g %.12g %.12g %.12g %.12g %.12g %.12g", x[i], y[i], mean_M[i], std::sqrt(var_M[i]), min_M[i], max_M[i],
                lppd[i], var_l[i]);
        for (size_t j = 0; j < Nq; j++) fprintf(o, " %.12g", qlo[j * (size_t)Nx + (size_t)i]);
        if (loo) fprintf(o, " %.12g %.12g", elpd[(size_t)i], khat[(size_t)i]);
        if (predictive) fprintf(o, " %.12g %.12g %.12g %.12g", pit[(size_t)i], log_cdf[(size_t)i], log_sf[(size_t)i], mean_resid[(size_t)i]);
        fprintf(o, "\n");
    }
    fclose(o);
    if (win_W) {
        const std::string win_file = out_file + ".windows";
        FILE *ow = fopen(win_file.c_str(), "w");
        if (!ow) return fail("unable to open the output file " + win_file);
        fprintf(ow, "# chainsummary_hip (%s)\n", tamcmc_version());
        fprintf(ow, "# W= %lld  first= %lld  n_windows= %lld\n", (long long)wt.W, (long long)wt.first, (long long)wt.n_windows);
        fprintf(ow, "# n_used= %lld  n_rejected= %lld\n", (long long)wt.n_used, (long long)wt.n_rejected);
        fprintf(ow, "# ks_D= %.12g  min_log_sf= %.12g  win_min_log_sf= %lld  min_log_cdf= %.12g  win_min_log_cdf= %lld\n", wt.ks_D, wt.min_log_sf,
                (long long)wt.win_min_log_sf, wt.min_log_cdf, (long long)wt.win_min_log_cdf);
        fprintf(ow, "# pit_hist=");
        for (int k = 0; k < TAMCMC_SUMMARY_PIT_CELLS; k++) fprintf(ow, " %lld", (long long)wt.pit_hist[k]);
        fprintf(ow, "\n# w first_bin last_bin x_first x_last pit log_cdf log_sf mean_resid\n");
        for (int64_t w = 0; w < wt.n_windows; w++) {
            const int64_t b = w == 0 ? 0 : wt.first + (w - 1) * wt.W, e = wt.first + w * wt.W < Nx ? wt.first + w * wt.W : Nx;
            fprintf(ow, "%lld %lld %lld %.12g %.12g %.12g %.12g %.12g %.12g\n", (long long)w, (long long)b, (long long)(e - 1), x[(size_t)b],
                    x[(size_t)(e - 1)], wpit[(size_t)w], wlog_cdf[(size_t)w], wlog_sf[(size_t)w], wmean_resid[(size_t)w]);
        }
        fclose(ow);
    }
    if (Ks) {
        const std::string scan_file = out_file + ".scan", reg_file = scan_file + ".regions";
        FILE *os = fopen(scan_file.c_str(), "w");
        if (!os) return fail("unable to open the output file " + scan_file);
        fprintf(os, "# chainsummary_hip (%s)\n", tamcmc_version());
        fprintf(os, "# widths= %s\n", scan_text.c_str());
        fprintf(os, "# n_used= %lld  n_rejected= %lld\n", (long long)st[0].n_used, (long long)st[0].n_rejected);
        for (size_t k = 0; k < Ks; k++)
            fprintf(os, "# W= %lld  n_positions= %lld  min_log_sf= %.17g  pos_min_log_sf= %lld  min_log_cdf= %.17g  pos_min_log_cdf= %lld\n",
                    (long long)st[k].W, (long long)st[k].n_positions, st[k].min_log_sf, (long long)st[k].pos_min_log_sf, st[k].min_log_cdf,
                    (long long)st[k].pos_min_log_cdf);
        fprintf(os, "# j x");
        for (size_t k = 0; k < Ks; k++) fprintf(os, " pit_%d log_cdf_%d log_sf_%d mean_resid_%d", (int)scan_W[k], (int)scan_W[k], (int)scan_W[k], (int)scan_W[k]);
        fprintf(os, "\n");
        for (int64_t j = 0; j < Nx; j++) {
            fprintf(os, "%lld %.17g", (long long)j, x[(size_t)j]);
            for (size_t k = 0; k < Ks; k++) {
                if (j >= st[k].n_positions) { fprintf(os, " nan nan nan nan"); continue; }
                for (int c = 0; c < 4; c++) fprintf(os, " %.17g", sarr[4 * k + c][(size_t)j]);
            }
            fprintf(os, "\n");
        }
        fclose(os);
        FILE *org = fopen(reg_file.c_str(), "w");
        if (!org) return fail("unable to open the output file " + reg_file);
        fprintf(org, "# chainsummary_hip (%s)\n", tamcmc_version());
        fprintf(org, "# widths= %s  log_below=", scan_text.c_str());
        if (null_R && !have_below) for (size_t i = 0; i < 2 * Ks; i++) fprintf(org, " %.17g", joint_line[i]);
        else for (size_t k = 0; k < Ks; k++) fprintf(org, " %.17g", have_below ? scan_below : std::log(0.01 * (double)scan_W[k] / (double)Nx));
        if (null_R) {
            fprintf(org, "\n# null= %lld %llu alpha= %.17g joint_line=", null_R, null_seed, null_alpha);
            for (size_t i = 0; i < 2 * Ks; i++) fprintf(org, " %.17g", joint_line[i]);
        }
        fprintf(org, "\n# W which pos_first pos_last bin_first bin_last x_first x_last pos_min min_log mean_resid_at_min%s\n", null_R ? " p_width p_joint" : "");
        for (size_t k = 0; k < Ks; k++)
            for (int which = 0; which < 2; which++) {
                const std::vector<tamcmc_summary_scan_region> &regs = sreg[2 * k + (size_t)which];
                for (size_t i = 0; i < regs.size(); i++) {
                    const tamcmc_summary_scan_region &r = regs[i];
                    fprintf(org, "%d %d %lld %lld %lld %lld %.17g %.17g %lld %.17g %.17g", (int)scan_W[k], which, (long long)r.pos_first,
                            (long long)r.pos_last, (long long)r.bin_first, (long long)r.bin_last, x[(size_t)r.bin_first], x[(size_t)r.bin_last],
                            (long long)r.pos_min, r.min_log, r.mean_resid_at_min);
                    if (null_R) fprintf(org, " %.17g %.17g", sreg_p[2 * k + (size_t)which][2 * i], sreg_p[2 * k + (size_t)which][2 * i + 1]);
                    fprintf(org, "\n");
                }
            }
        fclose(org);
    }
    if (loo_pit) {
        const std::string pit_file = out_file + ".loopit";
        FILE *op = fopen(pit_file.c_str(), "w");
        if (!op) return fail("unable to open the output file " + pit_file);
        fprintf(op, "# chainsummary_hip (%s)\n", tamcmc_version());
        fprintf(op, "# n_used= %lld  n_rejected= %lld\n", (long long)lpt.n_used, (long long)lpt.n_rejected);
        fprintf(op, "# ks_D= %.12g  min_log_sf= %.12g  bin_min_log_sf= %lld  min_log_cdf= %.12g  bin_min_log_cdf= %lld\n", lpt.ks_D, lpt.min_log_sf,
                (long long)lpt.bin_min_log_sf, lpt.min_log_cdf, (long long)lpt.bin_min_log_cdf);
        fprintf(op, "# min_is_ess= %.12g  bin_min_is_ess= %lld\n", lpt.min_is_ess, (long long)lpt.bin_min_is_ess);
        fprintf(op, "# pit_hist=");
        for (int k = 0; k < TAMCMC_SUMMARY_PIT_CELLS; k++) fprintf(op, " %lld", (long long)lpt.pit_hist[k]);
        fprintf(op, "\n# x loo_pit loo_log_cdf loo_log_sf is_ess pareto_k\n");
        for (int64_t i = 0; i < Nx; i++)
            fprintf(op, "%.12g %.12g %.12g %.12g %.12g %.12g\n", x[(size_t)i], lp_pit[(size_t)i], lp_cdf[(size_t)i], lp_sf[(size_t)i], lp_ess[(size_t)i],
                    khat[(size_t)i]);
        fclose(op);
    }
    if (lw_W) {
        const std::string lw_file = out_file + ".loowin";
        FILE *ol = fopen(lw_file.c_str(), "w");
        if (!ol) return fail("unable to open the output file " + lw_file);
        fprintf(ol, "# chainsummary_hip (%s)\n", tamcmc_version());
        fprintf(ol, "# W= %lld  first= %lld  n_windows= %lld\n", (long long)lwt.W, (long long)lwt.first, (long long)lwt.n_windows);
        fprintf(ol, "# n_used= %lld  n_rejected= %lld\n", (long long)lwt.n_used, (long long)lwt.n_rejected);
        fprintf(ol, "# elpd_lwo= %.12g  p_lwo= %.12g  k_max= %.12g  n_k_high= %lld  n_k_inf= %lld\n", lwt.elpd_lwo, lwt.p_lwo, lwt.k_max,
                (long long)lwt.n_k_high, (long long)lwt.n_k_inf);
        if (loo_pit) {
            fprintf(ol, "# ks_D= %.12g  min_log_sf= %.12g  win_min_log_sf= %lld  min_log_cdf= %.12g  win_min_log_cdf= %lld\n", lwpt.ks_D, lwpt.min_log_sf,
                    (long long)lwpt.bin_min_log_sf, lwpt.min_log_cdf, (long long)lwpt.bin_min_log_cdf);
            fprintf(ol, "# min_is_ess= %.12g  win_min_is_ess= %lld\n", lwpt.min_is_ess, (long long)lwpt.bin_min_is_ess);
            fprintf(ol, "# pit_hist=");
            for (int k = 0; k < TAMCMC_SUMMARY_PIT_CELLS; k++) fprintf(ol, " %lld", (long long)lwpt.pit_hist[k]);
            fprintf(ol, "\n");
        }
        fprintf(ol, "# first_bin last_bin x_first x_last elpd_lwo pareto_k tail_len%s\n", loo_pit ? " loo_pit loo_log_cdf loo_log_sf is_ess log_wsum" : "");
        for (size_t w = 0; w < lw_elpd.size(); w++) {
            fprintf(ol, "%lld %lld %.12g %.12g %.12g %.12g %d", (long long)lw_b[w], (long long)lw_e[w], x[(size_t)lw_b[w]], x[(size_t)lw_e[w]], lw_elpd[w],
                    lw_khat[w], (int)lw_tail[w]);
            if (loo_pit) fprintf(ol, " %.12g %.12g %.12g %.12g %.12g", lw_pit[w], lw_cdf[w], lw_sf[w], lw_ess[w], lw_wsum[w]);
            fprintf(ol, "\n");
        }
        fclose(ol);
    }
    if (ess_lag >= 0) {
        const std::string ess_file = out_file + ".ess";
        FILE *oe = fopen(ess_file.c_str(), "w");
        if (!oe) return fail("unable to open the output file " + ess_file);
        fprintf(oe, "# chainsummary_hip (%s)\n", tamcmc_version());
        fprintf(oe, "# n_used= %lld  n_rejected= %lld  lag= %lld\n", (long long)et.n_used, (long long)et.n_rejected, (long long)et.lag);
        fprintf(oe, "# min_ess_M= %.12g  bin_min_ess_M= %lld  min_ess_l= %.12g  bin_min_ess_l= %lld\n", et.min_ess_M, (long long)et.bin_min_ess_M,
                et.min_ess_l, (long long)et.bin_min_ess_l);
        fprintf(oe, "# max_rhat= %.12g  bin_max_rhat= %lld  n_rhat_high= %lld\n", et.max_rhat, (long long)et.bin_max_rhat, (long long)et.n_rhat_high);
        fprintf(oe, "# n_truncated_M= %lld  n_truncated_l= %lld\n", (long long)et.n_truncated_M, (long long)et.n_truncated_l);
        fprintf(oe, "# x ess_M tau_M mcse_M rhat_M cut_M ess_l r_eff cut_l\n");
        for (int64_t i = 0; i < Nx; i++)
            fprintf(oe, "%.12g %.12g %.12g %.12g %.12g %d %.12g %.12g %d\n", x[(size_t)i], ess_M[(size_t)i], tau_M[(size_t)i], mcse_M[(size_t)i],
                    rhat_M[(size_t)i], (int)cut_M[(size_t)i], ess_l[(size_t)i], r_eff[(size_t)i], (int)cut_l[(size_t)i]);
        fclose(oe);
    }
    if (band_lag >= 0) {
        const std::string band_file = out_file + ".bandess";
        FILE *ob = fopen(band_file.c_str(), "w");
        if (!ob) return fail("unable to open the output file " + band_file);
        fprintf(ob, "# chainsummary_hip (%s)\n", tamcmc_version());
        fprintf(ob, "# quantiles= %s\n", quant_text.c_str());
        fprintf(ob, "# n_used= %lld  n_rejected= %lld  lag= %lld\n", (long long)bt.n_used, (long long)bt.n_rejected, (long long)bt.lag);
        for (size_t j = 0; j < Nq; j++)
            fprintf(ob, "# q= %.6g  min_ess= %.12g  bin_min_ess= %lld  n_truncated= %lld  n_constant= %lld\n", quant[j], bt.min_ess[j],
                    (long long)bt.bin_min_ess[j], (long long)bt.n_truncated[j], (long long)bt.n_constant[j]);
        fprintf(ob, "# x");
        for (size_t j = 0; j < Nq; j++) {
            char q[32];
            snprintf(q, sizeof q, "%.6g", quant[j]);
            fprintf(ob, " q%s count_le_%s p_hat_%s ess_%s tau_%s mcse_p_%s cut_%s", q, q, q, q, q, q, q);
        }
        fprintf(ob, "\n");
        for (int64_t i = 0; i < Nx; i++) {
            fprintf(ob, "%.12g", x[(size_t)i]);
            for (size_t j = 0; j < Nq; j++) {
                const size_t at = j * (size_t)Nx + (size_t)i;
                fprintf(ob, " %.12g %d %.12g %.12g %.12g %.12g %d", qlo[at], (int)b_count[at], b_p[at], b_ess[at], b_tau[at], b_mcse[at], (int)b_cut[at]);
            }
            fprintf(ob, "\n");
        }
        fclose(ob);
    }
    if (modes) {
        static const char *const kind_name[] = {"inclination", "eta", "a3", "asymmetry", "freq", "width", "height", "amplitude", "splitting",
                                                "window_lo", "window_hi", "nu_m", "h_m"};
        const std::string modes_file = out_file + ".modes";
        FILE *om = fopen(modes_file.c_str(), "w");
        if (!om) return fail("unable to open the output file " + modes_file);
        fprintf(om, "# chainsummary_hip (%s)\n", tamcmc_version());
        fprintf(om, "# quantiles= %s\n", mquant_text.c_str());
        fprintf(om, "# n_used= %lld  n_rejected= %lld  n_cols= %lld  n_mult= %lld\n", (long long)mtt.n_used, (long long)mtt.n_rejected,
                (long long)mtt.n_cols, (long long)mtt.n_mult);
        fprintf(om, "# col kind mult order l m param_index mean sd min max");
        for (size_t j = 0; j < mquant.size(); j++) fprintf(om, " q%.6g", mquant[j]);
        fprintf(om, "\n");
        for (size_t k = 0; k < m_col.size(); k++) {
            const tamcmc_modetable_col &c = m_col[k];
            fprintf(om, "%zu %s %d %d %d %d %d %.17g %.17g %.17g %.17g", k, kind_name[c.kind], (int)c.mult, (int)c.order, (int)c.l, (int)c.m,
                    (int)c.param_index, m_mean[k], m_sd[k], m_min[k], m_max[k]);
            for (size_t j = 0; j < mquant.size(); j++) fprintf(om, " %.17g", m_q[j * m_col.size() + k]);
            fprintf(om, "\n");
        }
        fclose(om);
        if (modes_ess_lag >= 0) {
            const std::string ess_file = modes_file + ".ess";
            FILE *oe = fopen(ess_file.c_str(), "w");
            if (!oe) return fail("unable to open the output file " + ess_file);
            fprintf(oe, "# chainsummary_hip (%s)\n", tamcmc_version());
            fprintf(oe, "# n_used= %lld  n_rejected= %lld  n_cols= %lld  n_mult= %lld\n", (long long)mtt.n_used, (long long)mtt.n_rejected,
                    (long long)mtt.n_cols, (long long)mtt.n_mult);
            fprintf(oe, "# lag= %lld  min_ess= %.17g  col_min_ess= %lld  max_rhat= %.17g  col_max_rhat= %lld  n_truncated= %lld  n_constant= %lld  n_rhat_high= %lld\n",
                    (long long)mdt.lag, mdt.min_ess, (long long)mdt.col_min_ess, mdt.max_rhat, (long long)mdt.col_max_rhat, (long long)mdt.n_truncated,
                    (long long)mdt.n_constant, (long long)mdt.n_rhat_high);
            fprintf(oe, "# col kind mult order l m param_index ess tau mcse rhat cut\n");
            for (size_t k = 0; k < m_col.size(); k++) {
                const tamcmc_modetable_col &c = m_col[k];
                fprintf(oe, "%zu %s %d %d %d %d %d %.17g %.17g %.17g %.17g %d\n", k, kind_name[c.kind], (int)c.mult, (int)c.order, (int)c.l, (int)c.m,
                        (int)c.param_index, d_ess[k], d_tau[k], d_mcse[k], d_rhat[k], (int)d_cut[k]);
            }
            fclose(oe);
        }
        if (modes_corr) {
            const std::string corr_file = modes_file + ".corr";
            FILE *oc = fopen(corr_file.c_str(), "w");
            if (!oc) return fail("unable to open the output file " + corr_file);
            fprintf(oc, "# chainsummary_hip (%s)\n", tamcmc_version());
            fprintf(oc, "# n_used= %lld  n_rejected= %lld  n_cols= %lld  n_mult= %lld\n", (long long)mtt.n_used, (long long)mtt.n_rejected,
                    (long long)mtt.n_cols, (long long)mtt.n_mult);
            fprintf(oc, "# cols =");
            for (const int32_t k : head_cols) fprintf(oc, " %d", (int)k);
            fprintf(oc, "\n");
            const size_t nh = head_cols.size();
            for (size_t i = 0; i < nh; i++) {
                for (size_t j = 0; j < nh; j++) fprintf(oc, j ? " %.17g" : "%.17g", d_corr[i * nh + j]);
                fprintf(oc, "\n");
            }
            fclose(oc);
        }
        if (modes_rank_lag >= 0) {
            const std::string rank_file = modes_file + ".rank";
            FILE *orank = fopen(rank_file.c_str(), "w");
            if (!orank) return fail("unable to open the output file " + rank_file);
            fprintf(orank, "# chainsummary_hip (%s)\n", tamcmc_version());
            fprintf(orank, "# n_used= %lld  n_rejected= %lld  n_cols= %lld  n_mult= %lld\n", (long long)mtt.n_used, (long long)mtt.n_rejected,
                    (long long)mtt.n_cols, (long long)mtt.n_mult);
            fprintf(orank, "# lag= %lld  min_ess_bulk= %.17g  col_min_ess_bulk= %lld  min_ess_tail= %.17g  col_min_ess_tail= %lld  max_rhat= %.17g  "
                           "col_max_rhat= %lld  n_truncated= %lld  n_constant= %lld  n_rhat_high= %lld\n",
                    (long long)mrt.lag, mrt.min_ess_bulk, (long long)mrt.col_min_ess_bulk, mrt.min_ess_tail, (long long)mrt.col_min_ess_tail,
                    mrt.max_rhat, (long long)mrt.col_max_rhat, (long long)mrt.n_truncated, (long long)mrt.n_constant, (long long)mrt.n_rhat_high);
            fprintf(orank, "# col kind mult order l m param_index ess_bulk ess_tail rhat tau_bulk rhat_bulk rhat_fold ess_q05 ess_q95 cut_z cut_zfold cut_i05 cut_i95\n");
            const size_t nc = m_col.size();
            for (size_t k = 0; k < nc; k++) {
                const tamcmc_modetable_col &c = m_col[k];
                fprintf(orank, "%zu %s %d %d %d %d %d", k, kind_name[c.kind], (int)c.mult, (int)c.order, (int)c.l, (int)c.m, (int)c.param_index);
                for (size_t j = 0; j < TAMCMC_MODERANK_NOUT; j++) fprintf(orank, " %.17g", r_out[j * nc + k]);
                for (size_t j = 0; j < TAMCMC_MODERANK_NSERIES; j++) fprintf(orank, " %d", (int)r_cut[j * nc + k]);
                fprintf(orank, "\n");
            }
            fclose(orank);
        }
        auto pdf_open = [&](const std::string &name) {
            FILE *f = fopen(name.c_str(), "w");
            if (!f) return f;
            fprintf(f, "# chainsummary_hip (%s)\n", tamcmc_version());
            fprintf(f, "# n_used= %lld  n_rejected= %lld  n_cols= %lld  n_mult= %lld\n", (long long)mtt.n_used, (long long)mtt.n_rejected,
                    (long long)mtt.n_cols, (long long)mtt.n_mult);
            return f;
        };
        if (hist_bins != 0) {
            const std::string hist_file = modes_file + ".hist";
            FILE *oh = pdf_open(hist_file);
            if (!oh) return fail("unable to open the output file " + hist_file);
            fprintf(oh, "# n_bins= %ld\n", hist_bins);
            for (size_t k = 0; k < m_col.size(); k++) {
                const tamcmc_modetable_col &c = m_col[k];
                const double lo = h_range[2 * k], hi = h_range[2 * k + 1];
                fprintf(oh, "# col %zu %s %d %d %d %d %d\n", k, kind_name[c.kind], (int)c.mult, (int)c.order, (int)c.l, (int)c.m, (int)c.param_index);
                fprintf(oh, "# range= %.17g %.17g  status= %d\n", lo, hi, (int)h_status[k]);
                fprintf(oh, "# below= %lld  above= %lld\n", (long long)h_below[k], (long long)h_above[k]);
                for (long b = 0; b < hist_bins; b++)     // the plot edge of tamcmc_accel_pdf.h: lo + (hi - lo) * (b / n_bins)
                    fprintf(oh, "%.17g %lld\n", lo + (hi - lo) * ((double)b / (double)hist_bins), (long long)h_cnt[k * (size_t)hist_bins + (size_t)b]);
                fprintf(oh, "%.17g\n", hi);
            }
            fclose(oh);
        }
        if (!hpd_mass.empty()) {
            const std::string hpd_file = modes_file + ".hpd";
            FILE *op = pdf_open(hpd_file);
            if (!op) return fail("unable to open the output file " + hpd_file);
            const size_t nm = hpd_mass.size(), nc = m_col.size();
            fprintf(op, "# mass= %s\n# k=", hpd_text.c_str());
            for (size_t m = 0; m < nm; m++) fprintf(op, " %lld", (long long)p_k[m]);
            fprintf(op, "\n# col kind mult order l m param_index median");
            for (size_t m = 0; m < nm; m++) fprintf(op, " k%.6g lo%.6g hi%.6g", hpd_mass[m], hpd_mass[m], hpd_mass[m]);
            fprintf(op, "\n");
            for (size_t k = 0; k < nc; k++) {
                const tamcmc_modetable_col &c = m_col[k];
                fprintf(op, "%zu %s %d %d %d %d %d %.17g", k, kind_name[c.kind], (int)c.mult, (int)c.order, (int)c.l, (int)c.m, (int)c.param_index, p_med[k]);
                for (size_t m = 0; m < nm; m++) fprintf(op, " %lld %.17g %.17g", (long long)p_k[m], p_lo[m * nc + k], p_hi[m * nc + k]);
                fprintf(op, "\n");
            }
            fclose(op);
        }
        if (!pair_cols.empty()) {
            const std::string pairs_file = modes_file + ".pairs";
            FILE *oj = pdf_open(pairs_file);
            if (!oj) return fail("unable to open the output file " + pairs_file);
            const size_t np = pair_cols.size() / 2, nb = (size_t)pair_bins;
            fprintf(oj, "# n_bins= %ld\n", pair_bins);
            for (size_t p = 0; p < np; p++) {
                fprintf(oj, "# pair %d %d\n", (int)pair_cols[2 * p], (int)pair_cols[2 * p + 1]);
                fprintf(oj, "# range= %.17g %.17g %.17g %.17g  status= %d\n", j_range[4 * p], j_range[4 * p + 1], j_range[4 * p + 2], j_range[4 * p + 3],
                        (int)j_status[p]);
                fprintf(oj, "# outside= %lld  level68= %lld  level95= %lld\n", (long long)j_out[p], (long long)j_level[p], (long long)j_level[np + p]);
                for (size_t a = 0; a < nb; a++) {
                    for (size_t b = 0; b < nb; b++) fprintf(oj, b ? " %lld" : "%lld", (long long)j_cnt[(p * nb + a) * nb + b]);
                    fprintf(oj, "\n");
                }
            }
            fclose(oj);
        }
        if (modes_indices) {
            static const char *const index_name[] = {"dnu_fit", "epsilon", "numax", "dnu_nl", "d2nu", "d02", "d13", "d01", "d10", "r02", "r01", "r13", "r10"};
            const size_t nb = (size_t)sinfo.n_base_cols, ni = (size_t)sinfo.n_index_cols, na = nb + ni;
            const std::string ind_file = modes_file + ".indices";
            FILE *oi = fopen(ind_file.c_str(), "w");
            if (!oi) return fail("unable to open the output file " + ind_file);
            fprintf(oi, "# chainsummary_hip (%s)\n", tamcmc_version());
            fprintf(oi, "# quantiles= %s\n", mquant_text.c_str());
            fprintf(oi, "# n_used= %lld  n_rejected= %lld  n_base_cols= %lld  n_index_cols= %lld  n_radial= %lld  n_unassigned= %lld  n_base= %lld  dnu_ref= %.17g  eps_ref= %.17g\n",
                    (long long)stt.n_used, (long long)stt.n_rejected, (long long)sinfo.n_base_cols, (long long)sinfo.n_index_cols, (long long)sinfo.n_radial,
                    (long long)sinfo.n_unassigned, (long long)sinfo.n_base, sinfo.dnu_ref, sinfo.eps_ref);
            fprintf(oi, "# col kind l n mean sd");
            for (size_t j = 0; j < mquant.size(); j++) fprintf(oi, " q%.6g", mquant[j]);
            if (modes_ess_lag >= 0) fprintf(oi, " ess tau mcse rhat cut");
            if (modes_rank_lag >= 0) fprintf(oi, " ess_bulk ess_tail rhat_rank tau_bulk rhat_bulk rhat_fold ess_q05 ess_q95 cut_z cut_zfold cut_i05 cut_i95");
            fprintf(oi, "\n");
            for (size_t k = nb; k < na; k++) {
                const tamcmc_modetable_col &c = s_col[k];
                fprintf(oi, "%zu %s %d %d %.17g %.17g", k, index_name[c.kind - TAMCMC_MODETABLE_DNU_FIT], (int)c.l, (int)c.order, s_mean[k], s_sd[k]);
                for (size_t j = 0; j < mquant.size(); j++) fprintf(oi, " %.17g", s_q[j * na + k]);
                if (modes_ess_lag >= 0) fprintf(oi, " %.17g %.17g %.17g %.17g %d", s_ess[k], s_tau[k], s_mcse[k], s_rhat[k], (int)s_cut[k]);
                if (modes_rank_lag >= 0) {
                    for (size_t j = 0; j < TAMCMC_MODERANK_NOUT; j++) fprintf(oi, " %.17g", s_rout[j * ni + (k - nb)]);
                    for (size_t j = 0; j < TAMCMC_MODERANK_NSERIES; j++) fprintf(oi, " %d", (int)s_rcut[j * ni + (k - nb)]);
                }
                fprintf(oi, "\n");
            }
            fclose(oi);
            const std::string cov_file = ind_file + ".cov";
            FILE *oc = fopen(cov_file.c_str(), "w");
            if (!oc) return fail("unable to open the output file " + cov_file);
            fprintf(oc, "# chainsummary_hip (%s)\n", tamcmc_version());
            fprintf(oc, "# n_used= %lld  n_rejected= %lld  n_base_cols= %lld  n_index_cols= %lld\n", (long long)stt.n_used, (long long)stt.n_rejected,
                    (long long)sinfo.n_base_cols, (long long)sinfo.n_index_cols);
            fprintf(oc, "# cols =");
            for (const int32_t k : ratio_cols) fprintf(oc, " %d", (int)k);
            fprintf(oc, "\n# rows =");
            for (const int32_t k : ratio_cols) fprintf(oc, " %s_n%d", index_name[s_col[(size_t)k].kind - TAMCMC_MODETABLE_DNU_FIT], (int)s_col[(size_t)k].order);
            fprintf(oc, "\n");
            const size_t nr = ratio_cols.size();
            for (size_t i = 0; i < nr; i++) {
                for (size_t j = 0; j < nr; j++) fprintf(oc, j ? " %.17g" : "%.17g", s_cov[i * nr + j]);
                fprintf(oc, "\n");
            }
            fclose(oc);
        }
    }
    printf("Summary of %lld samples (%lld rejected) written to %s\n", (long long)t.n_used, (long long)t.n_rejected, out_file.c_str());
    return 0;
}
