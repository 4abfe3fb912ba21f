// sh_k2_tx.h - translated search (DESIGN.md §7 "Translated search"): the rules of the six-frame translation and of the amino-acid
// alphabet, shared by sh_k2_tx.hip (k_k2_translate, the residue-to-code pass, the host mirror) and sh_k2.hip (the protein form of
// k_k2_classify computes the same frame extents).  aa_translate.cc and mmscanner.cc as recalled: PARITY UNPINNED, like the rest of §7.
#pragma once
#include "sh_common.h"

#define K2_AA_AMBIG 0x80u       // a code byte outside 0..15: restarts the l-mer and the window, as a non-ACGT base does

// ResolveTree's threshold over a protein database is ceil(confidence * (total_kmers + S)).  Kraken 2 counts its frame-border
// markers in taxa.size(): 5 for a read, 11 for a pair; it then subtracts 2 for a read, and 4 + 1 for a pair.
#define K2_TX_S_READ 3u
#define K2_TX_S_PAIR 6u

// residues of the three forward frames of a record of n bases (the reverse frames have as many): frame f holds the codons that
// end at the bases i >= 2 with i % 3 == f, so the codons that start at base 0 land in frame 2
__host__ __device__ static inline void k2_tx_frame_lens(uint64_t n, uint64_t &n0, uint64_t &n1, uint64_t &n2)
{
    n0 = n >= 3 ? (n - 1) / 3 : 0; n1 = n >= 3 ? (n - 2) / 3 : 0; n2 = n >= 3 ? n / 3 : 0;
}

// A=0 C=1 G=2 T=3, either letter case; 4 = anything else
__host__ __device__ static inline uint32_t k2_tx_nt(uint32_t ch)
{
    const uint32_t u = ch | 0x20u;
    return u == 'a' ? 0u : u == 'c' ? 1u : u == 'g' ? 2u : u == 't' ? 3u : 4u;
}
// the standard code, indexed by 16 * b0 + 4 * b1 + b2: the 64 residues packed eight to a word so that the table lives in
// registers / literals on either side (no array, no constant memory)
__host__ __device__ static inline uint32_t k2_tx_residue(uint32_t codon)
{
    //                      "KNKNTTTT" "RSRSIIMI" "QHQHPPPP" "RRRRLLLL" "EDEDAAAA" "GGGGVVVV" "*Y*YSSSS" "*CWCLFLF"
    const uint64_t w = codon < 8 ? 0x545454544e4b4e4bull : codon < 16 ? 0x494d494953525352ull : codon < 24 ? 0x5050505048514851ull
                     : codon < 32 ? 0x4c4c4c4c52525252ull : codon < 40 ? 0x4141414144454445ull : codon < 48 ? 0x5656565647474747ull
                     : codon < 56 ? 0x53535353592a592aull : 0x464c464c4357432aull;
    return (uint32_t)(w >> (8 * (codon & 7u))) & 0xffu;
}
// the reduced 15-letter alphabet in 4 bits, either letter case: *UO 0, A 1, NQS 2, C 3, DE 4, F 5, G 6, H 7, IL 8, K 9, P 10, R 11,
// MV 12, T 13, W 14, Y 15; every other byte (X, B, J, Z included) K2_AA_AMBIG.  The 26 letters' codes, 5 bits each (31 = none),
// sit in three words.
__host__ __device__ static inline uint32_t k2_aa_code(uint32_t ch)
{
    if (ch == '*') return 0u;
    const uint32_t u = (ch | 0x20u) - 'a';
    if (u >= 26u) return K2_AA_AMBIG;
    //              A  B   C  D  E  F  G  H  I  J   | K  L  M   N  O  P   Q  R   S  T   | U  V   W   X   Y   Z
    const uint64_t a = 1ull | 31ull << 5 | 3ull << 10 | 4ull << 15 | 4ull << 20 | 5ull << 25 | 6ull << 30 | 7ull << 35 | 8ull << 40 | 31ull << 45;
    const uint64_t b = 9ull | 8ull << 5 | 12ull << 10 | 2ull << 15 | 0ull << 20 | 10ull << 25 | 2ull << 30 | 11ull << 35 | 2ull << 40 | 13ull << 45;
    const uint64_t c = 0ull | 12ull << 5 | 14ull << 10 | 31ull << 15 | 15ull << 20 | 31ull << 25;
    const uint32_t v = (uint32_t)((u < 10 ? a >> (5 * u) : u < 20 ? b >> (5 * (u - 10)) : c >> (5 * (u - 20))) & 31u);
    return v == 31u ? K2_AA_AMBIG : v;
}

// k_k2_translate over a batch whose extent (beg = offsets[0], n_bases = offsets[n_records] - beg) the caller knows: d_out holds
// 2 * n_bases + 8 bytes; enqueued on s, no synchronisation
sh_status shi_k2_translate_device(const uint8_t *d_bases, const uint8_t *d_quals, const uint64_t *d_offsets, uint64_t n_records, uint64_t beg, uint64_t n_bases,
                                  int32_t min_qual, int32_t as_letters, uint8_t *d_out, hipStream_t s);
// a protein library's residues to scanner codes: d_codes[i] = k2_aa_code(d_residues[i]) for i < n; the two arrays lie at the same
// address modulo 8 (else SH_ERR_BAD_ARG); enqueued on s, no synchronisation
sh_status shi_k2_aa_encode_device(const uint8_t *d_residues, uint8_t *d_codes, uint64_t n, hipStream_t s);
