// sh_k2_db.h - the Kraken arm's database handle and the two walks over its taxonomy, shared by sh_k2.hip (build, classify, files),
// sh_k2_inspect.hip (inspection) and sh_k2_distrib.hip (window calls)
#pragma once
#include "sh_common.h"

struct sh_k2_db {
    int device = 0;
    sh_k2_opts opts{};
    uint64_t capacity = 0, size = 0;
    int32_t key_bits = 0, value_bits = 0;
    uint32_t *d_cells = nullptr, *d_parent = nullptr, *d_ext = nullptr;
    unsigned long long *d_ctr = nullptr;         // [0] new cells claimed, [1] table full
    std::vector<sh_k2_taxnode> nodes;
    std::string names, ranks;
    // opts.k2d fields carried through save/open
    int32_t dna_db = 1, revcom_version = 1, db_version = 0, db_type = 0;
};

// breadth-first ids: a parent's id is smaller than its child's; 0 is no taxon
__device__ static inline uint32_t k2_lca(const uint32_t *__restrict__ parent, uint32_t a, uint32_t b)
{
    if (!a || !b) return a ? a : b;
    while (a != b) { if (a > b) a = parent[a]; else b = parent[b]; }
    return a;
}
__device__ static inline bool k2_is_ancestor(const uint32_t *__restrict__ parent, uint32_t a, uint32_t b)
{
    if (!a || !b) return false;
    while (b > a) b = parent[b];
    return a == b;
}

// kraken2 --minimum-base-quality (MaskLowQualityBases): Phred score below the threshold; 0xFF = a FASTA record, never masked
__host__ __device__ static inline bool k2_masked(uint32_t q, int32_t min_qual)
{
    return q != 0xffu && (int32_t)q - '!' < min_qual;
}
