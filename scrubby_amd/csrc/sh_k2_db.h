// sh_k2_db.h - the Kraken arm's database handle, shared by sh_k2.hip (build, classify, files) and sh_k2_inspect.hip (inspection)
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
