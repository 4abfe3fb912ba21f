// sh_k2_inspect.h - internal entry points of sh_k2_inspect.hip (database inspection, DESIGN.md §7 "Database inspection")
#pragma once
#include "sh_common.h"

// The tree walk of both reports (sh_k2_write_report's per-read calls, sh_k2_counts_report's per-cell counts): depth-first from the
// root, children by clade count (descending; ties by id), rank codes with a depth suffix.  clade / direct: n entries; parents have
// smaller ids than their children.  names / ranks: the NUL-terminated pools of taxo.k2d.  flags: SH_K2_INSPECT_ZERO_COUNTS (also the
// taxa whose clade count is 0), SH_K2_INSPECT_MPA.  extra_a / extra_b (both or neither): two more per-taxon columns after `direct`
// in the Kraken-style rows (sh_k2_write_minimizer_report).
void shi_k2_report_rows(FILE *f, const sh_k2_taxnode *nodes, size_t n, const std::string &names, const std::string &ranks, const uint64_t *clade,
                        const uint64_t *direct, double total, int32_t flags, const uint64_t *extra_a = nullptr, const uint64_t *extra_b = nullptr);
