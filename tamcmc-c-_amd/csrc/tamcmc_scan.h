// tamcmc_scan.h -- sliding-window predictive scan of a stored chain (tamcmc_summary_scan_* in include/tamcmc_accel.h): the
// windowed check of tamcmc_window.h at EVERY start position and for up to TM_SCAN_MAX_WIDTHS widths at once, in the pass the
// user already makes.  A feature cut by a boundary of the disjoint windows is whole in some window of the scan, and a user
// who does not know the width of what they look for pays one pass, not one per trial width.
//
//   widths       W_0 < ... < W_{K-1}, each 1 ... TM_WIN_MAX_BINS and at most Nx.  Width k has the positions j = 0 ... Nx - W_k,
//                n_pos_k = Nx - W_k + 1 of them; the window of position j is the bins [j, j + W_k): every window is full.
//   sums, tails  per (sample, width, position) exactly the disjoint check's: tmw_sum over q + j, tmw_chi / tmw_gauss with the
//                one shape tmw_shape(W_k, p) of the width.  A scan window is a full window of the disjoint check with some
//                (W, first) and equals it bit for bit.  The sums of all widths at one position are the prefixes of ONE ascending
//                sum started at q[j] -- tmw_sum's own additions in its own order -- so one walk serves every width.
//                (A running prefix-difference sum would be cheaper and round differently: not wanted.)
//   fold         per (width, position) over the accepted samples in push order: the window fold kernel's walk with
//                (double)W_k for the length.
//   state        TM_PRED_NSTATE blocks of total = sum_k n_pos_k doubles; width k's positions start at off_k = sum_{k' < k} n_pos_k'.
//   scratch      [3][C][total] doubles -- log P, log Q and the sum of every (sample, width, position) of a chunk of
//                C = max(1, min(block_chains, TM_SCAN_CHUNK_MAX, TM_SCAN_SCRATCH_BYTES / (24 total))) samples.  A block with
//                more samples is worked in chunks of C, the fold kernel going on from the stored state with the count of
//                the accepted samples before the chunk: that cannot change a bit.
//
// The host-only arithmetic below (position counts, chunk size, default line, region finder) is plain C++17, callable from g++
// (tests/cpp/scan_core_check.cpp).
#pragma once
#include "tamcmc_window.h"

#define TM_SCAN_MAX_WIDTHS 8      // TAMCMC_SUMMARY_SCAN_MAX_WIDTHS
#define TM_SCAN_THREADS 256
#define TM_SCAN_TILE 2048         // positions of one sample a workgroup of the sums kernel works on
// the tile's residuals and the halo the widest window of its last position reaches into: 2559 doubles, 20 472 bytes
#define TM_SCAN_LDS_DOUBLES (TM_SCAN_TILE + TM_WIN_MAX_BINS - 1)
#define TM_SCAN_CHUNK_MAX 4096
#define TM_SCAN_SCRATCH_BYTES ((long long)256 << 20)

// ---- host-only arithmetic ----

inline long long tmsc_positions(const long long Nx, const int W) { return Nx - W + 1; }

// the offsets off[0 ... K-1] of the widths' positions on the concatenated axis; returns total = sum_k n_pos_k
inline long long tmsc_layout(const long long Nx, const int K, const int32_t *W, long long *off)
{
    long long total = 0;
    for (int k = 0; k < K; k++) {
        off[k] = total;
        total += tmsc_positions(Nx, W[k]);
    }
    return total;
}

// samples per chunk
inline long long tmsc_chunk(const long long block_chains, const long long total)
{
    long long c = block_chains < TM_SCAN_CHUNK_MAX ? block_chains : TM_SCAN_CHUNK_MAX;
    const long long fit = TM_SCAN_SCRATCH_BYTES / (24 * total);
    c = c < fit ? c : fit;
    return c < 1 ? 1 : c;
}

// the Bonferroni line at 1 % over Nx / W independent windows
inline double tmsc_default_line(const int W, const long long Nx) { return log(0.01 * (double)W / (double)Nx); }

struct TmScanRegion {             // tamcmc_summary_scan_region, field for field
    int64_t pos_first, pos_last, bin_first, bin_last, pos_min;
    double min_log, mean_resid_at_min;
};

// The maximal runs of consecutive positions with v[j] < line (a NaN is never below it), in position order: the count of
// all of them; the first max_regions are written to out (which may be NULL when max_regions is 0).  pos_min is the first
// position of the run's minimum.
inline long long tmsc_regions(const double *v, const double *mean_resid, const long long n_pos, const int W, const double line,
                              const long long max_regions, TmScanRegion *out)
{
    long long count = 0;
    for (long long j = 0; j < n_pos;) {
        if (!(v[j] < line)) { j++; continue; }
        TmScanRegion r;
        r.pos_first = j; r.pos_min = j; r.min_log = v[j];
        for (j++; j < n_pos && v[j] < line; j++)
            if (v[j] < r.min_log) { r.min_log = v[j]; r.pos_min = j; }
        r.pos_last = j - 1;
        r.bin_first = r.pos_first;
        r.bin_last = r.pos_last + W - 1;
        r.mean_resid_at_min = mean_resid[r.pos_min];
        if (count < max_regions) out[count] = r;
        count++;
    }
    return count;
}

// ---- launch arguments (tamcmc_scan.hip) ----
struct TmScanArgs {
    const double *rows;           // [B][Nx] model rows of the block (stage 1)
    const int32_t *status;        // [B]
    const double *y, *isig2;      // as TmSummaryArgs
    double *state;                // [TM_PRED_NSTATE][total]
    double *scratch;              // [3][C][total]: log P, log Q, the sum, of every (sample, width, position) of a chunk
    const long long *cnt_in;      // {accepted, rejected} before this block: the pair the block's fold launch read
    long long total;              // sum_k n_pos_k
    long long off[TM_SCAN_MAX_WIDTHS];
    int32_t W[TM_SCAN_MAX_WIDTHS];
    int32_t Nx, B;
    int32_t C;                    // samples per chunk: the scratch's stride
    int32_t K;
    int32_t likelihood_case, p;
    TmWinShape shape[TM_SCAN_MAX_WIDTHS];
};

// per chunk of the block the sums kernel, the tails kernel and the fold kernel, in that order on `stream`; returns a hipError_t
int tm_launch_scan(const TmScanArgs &a, void *stream);
