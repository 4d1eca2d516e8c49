// What fdr.hip (Benjamini-Hochberg along rows) shares with fdr_scope.hip (along columns, over the whole matrix): the row
// adjustment itself, the read-only count-ratio check and the NES epilogue.  Each is defined ONCE, in fdr.hip, beside its kernels
// (every kernel is launched from its own translation unit).
#pragma once
#include "common.h"

// Benjamini-Hochberg on every row of p_dev (f64 [n, m] row-major) in place.  n_perm > 0: the caller has checked that every entry
// is a count ratio c / n_perm (fdr_all_count_ratios) -- rows are adjusted from their histograms where the table fits the LDS;
// n_perm = 0: the rows are sorted.  The stream has drained when it returns.
int fdr_matrix(safe_ctx *ctx, double *p_dev, int64_t n, int64_t m, int64_t n_perm = 0);

// *all = every non-NaN entry of the n_mats matrices of `total` entries each is c / n_perm with c in [0, n_perm] (k_fdr_check_ratio).
// Reads only; the stream has drained when it returns.
int fdr_all_count_ratios(safe_ctx *ctx, const double *const *mats, int n_mats, int64_t total, int64_t n_perm, bool *all);

// nes, nes_binary and the per-attribute counts from (adjusted) p-values: k_nes_from_pvalues, the tail of safe_fdr_adjust.
// `who` names the entry point in error messages.  The stream has drained when it returns.
int fdr_nes_epilogue(safe_ctx *ctx, const char *who, int64_t n, int64_t m, int64_t num_permutations, int sign_mode,
                     double enrichment_threshold, const double *pvalues_neg_dev, const double *pvalues_pos_dev, double *nes_dev,
                     double *nes_binary_dev, double *num_enriched_dev);
