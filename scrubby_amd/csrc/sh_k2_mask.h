// sh_k2_mask.h - internal entry points of sh_k2_mask.hip (low-complexity masking)
#pragma once
#include "sh_common.h"

// window / threshold 0 -> 64 / 20; refuses a window outside [8, 64], a threshold < 1, a replacement that is no byte
sh_status shi_k2_mask_params(int32_t *window, int32_t *threshold, int32_t replacement, const char *who);
// sh_k2_mask_device for a batch whose first or last record is a piece of a record that the library reader cut: n_masked leaves
// out the first quiet_head and the last quiet_tail bases of the batch (context only, or counted by the piece before the cut)
sh_status shi_k2_mask_device(uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_records, int32_t window, int32_t threshold, int32_t replacement,
                             uint64_t quiet_head, uint64_t quiet_tail, hipStream_t s, sh_k2_mask_stats *stats);
