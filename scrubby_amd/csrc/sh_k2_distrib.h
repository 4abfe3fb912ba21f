// sh_k2_distrib.h - what sh_k2.hip (the scanner and the probe) and sh_k2_distrib.hip (windows, accumulator, estimate) share
// (DESIGN.md §7 "Abundance re-estimation")
#pragma once
#include "sh_common.h"
#include "sh_k2_db.h"

// One code per k-mer of a batch, as the hit lists have them: k-mer j of record r (bases j .. j + k - 1) at d_codes[d_offsets[r] + j];
// internal taxon, 0 (not in the table, not looked up, or a cell value outside the taxonomy) or SH_K2_HIT_AMBIGUOUS.  Records whose
// taxon is 0 or >= n_nodes and records shorter than k get none.  d_seg: n_records + 1 words of scratch, tmp: the scan's scratch; both
// must outlive the stream's work.  A batch of more than codes_cap bases writes nothing but its size to *d_need (the caller grows
// d_codes and calls again).  Everything on stream s, no synchronisation.
sh_status shi_k2_codes_device(const sh_k2_db *db, const uint8_t *d_bases, const uint64_t *d_offsets, const uint32_t *d_taxa, uint64_t n_records,
                              uint64_t *d_seg, DevBuf &tmp, uint32_t *d_codes, uint64_t codes_cap, unsigned long long *d_need, hipStream_t s);

