// sh_k2_inspect.hip - what is IN a database (DESIGN.md §7 "Database inspection"): kraken2-inspect's header lines and its per-taxon
// minimizer counts, as recalled from dump_table.cc and CompactHashTable::GetValueCounts (PARITY UNPINNED).
//
// k_k2_value_counts: one pass over cells[capacity] in HBM and a histogram by value into counts[n_nodes] (uint64).
//   loads       a persistent grid (blocks of 256 threads, K2I_BLOCKS_PER_CU per CU) strides over the table; a trip of a block is
//               K2I_UNROLL x 256 lanes x 16 bytes (four cells per lane and load), cell indices are 64-bit.  Only the capacity / 4 whole
//               vectors are loaded that way; the last capacity % 4 cells are read one by one, so no load touches a byte behind the table.
//   cells       a cell that is 0 is empty.  An occupied cell whose value (its low value_bits bits) is 0 or >= n_nodes is a bad value:
//               it counts in n_bad_values and its value becomes 0 before anything else looks at it, and k2i_add - the only place that
//               adds - compares the value with 0 and n_nodes once more in front of both of its adds.
//   contention  (1) uniform wave: when every countable cell of a wave's load holds the same value (one readlane of the first such
//               lane's value, one ballot), ONE lane adds the population count: 1 add per 256 cells in a single-taxon table;
//               (2) otherwise a lane merges its own four cells where they are equal and adds once per distinct value;
//               (3) values below lds_bins (<= K2I_LDS_BINS; breadth-first ids put the root and the hot LCAs there) go to 32-bit
//               bins of the block in LDS, flushed to HBM with one 64-bit add per non-zero bin; the others are 64-bit no-return adds
//               in HBM.
//   overflow    a 32-bit LDS bin cannot overflow at any capacity because the cells a block handles between two flushes are BOUNDED:
//               it flushes after every K2I_FLUSH_TRIPS trips = 2^30 cells (+ at most 3 of the ragged end), below 2^32.
// Integer adds only: the result is exact and does not depend on the order of the adds.
#include "sh_common.h"
#include "sh_k2_db.h"
#include "sh_k2_inspect.h"
#include "sh_wave.h"
#include <algorithm>
#include <chrono>
#include <cstdlib>

#define K2I_THREADS 256u
#define K2I_UNROLL 2u
#define K2I_BLOCKS_PER_CU 8u            // 32 waves per CU; 8 x 16 KiB of bins fit the 160 KiB of LDS
#define K2I_LDS_BINS 4096u              // bin limit: 16 KiB per block
#define K2I_LDS_BINS_MAX 16384u         // what the switch may ask for: 64 KiB, one block's LDS without an opt-in
#define K2I_FLUSH_TRIPS (1u << 19)      // x K2I_UNROLL * 256 * 4 = 2048 cells per trip = 2^30 cells between two flushes

struct K2InspectArgs {
    const uint32_t *cells; uint64_t capacity;
    uint32_t vmask, n_nodes, lds_bins;
    unsigned long long *counts;        // n_nodes, zero at launch
    unsigned long long *ctr;           // nullable: [0] occupied cells, [1] bad values
};

// the only place that adds: w cells of value v
__device__ static inline void k2i_add(uint32_t *bins, const K2InspectArgs &a, uint32_t v, uint32_t w)
{
    if (v == 0u || v >= a.n_nodes) return;           // a value never becomes an index unchecked
    if (v < a.lds_bins) __hip_atomic_fetch_add(&bins[v], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_fetch_add(&a.counts[v], (unsigned long long)w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// empty -> 0 and nothing counted; bad value -> 0, counted in occ and bad; else the value, counted in occ
__device__ static inline uint32_t k2i_value(uint32_t cell, const K2InspectArgs &a, uint32_t &occ, uint32_t &bad)
{
    const uint32_t t = cell & a.vmask;
    const bool o = cell != 0u, g = o && t != 0u && t < a.n_nodes;
    occ += o; bad += o && !g;
    return g ? t : 0u;
}

// the four cells of one lane's load; the whole wave is here (a lane behind the last vector holds four empty cells)
__device__ static inline void k2i_vec(const uint4 c, uint32_t lane, uint32_t *bins, const K2InspectArgs &a, uint32_t &occ, uint32_t &bad)
{
    const uint32_t v0 = k2i_value(c.x, a, occ, bad), v1 = k2i_value(c.y, a, occ, bad), v2 = k2i_value(c.z, a, occ, bad), v3 = k2i_value(c.w, a, occ, bad);
    const uint32_t r = v0 ? v0 : v1 ? v1 : v2 ? v2 : v3;                       // the lane's first countable value
    const uint64_t have = __ballot(r != 0u);
    if (have == 0) return;
    const int leader = __ffsll((unsigned long long)have) - 1;
    const uint32_t first = (uint32_t)wave_bcast((int32_t)r, leader);
    const bool other = (v0 && v0 != first) || (v1 && v1 != first) || (v2 && v2 != first) || (v3 && v3 != first);
    if (__ballot(other) == 0) {                                                // uniform wave: one add of the population count
        const uint32_t total = (uint32_t)(__popcll(__ballot(v0 != 0u)) + __popcll(__ballot(v1 != 0u)) + __popcll(__ballot(v2 != 0u)) + __popcll(__ballot(v3 != 0u)));
        if ((int)lane == leader) k2i_add(bins, a, first, total);
        return;
    }
    // the lane's own cells: the first cell of each distinct value carries the count of its equals
    const bool e01 = v0 == v1, e02 = v0 == v2, e03 = v0 == v3, e12 = v1 == v2, e13 = v1 == v3, e23 = v2 == v3;
    if (v0) k2i_add(bins, a, v0, 1u + e01 + e02 + e03);
    if (v1 && !e01) k2i_add(bins, a, v1, 1u + e12 + e13);
    if (v2 && !e02 && !e12) k2i_add(bins, a, v2, 1u + e23);
    if (v3 && !e03 && !e13 && !e23) k2i_add(bins, a, v3, 1u);
}

// every thread of the block: the non-zero bins go to HBM with one 64-bit add each and start again at 0
__device__ static inline void k2i_flush(uint32_t *bins, const K2InspectArgs &a)
{
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < a.lds_bins; b += K2I_THREADS) {
        const uint32_t n = bins[b];
        if (n) { __hip_atomic_fetch_add(&a.counts[b], (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); bins[b] = 0; }
    }
    __syncthreads();
}

__global__ __launch_bounds__(K2I_THREADS) void k_k2_value_counts(K2InspectArgs a)
{
    extern __shared__ uint32_t s_bins[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t b = tid; b < a.lds_bins; b += K2I_THREADS) s_bins[b] = 0;
    __syncthreads();
    const uint64_t n_vec = a.capacity >> 2;                       // whole 16-byte vectors; the table is 16-byte aligned (hipMalloc)
    const uint4 *vec = (const uint4 *)a.cells;
    const uint64_t per_trip = (uint64_t)K2I_THREADS * K2I_UNROLL;
    unsigned long long occ = 0, bad = 0;
    uint32_t trips = 0;
    // the loop bounds are the same for every thread of the block (k2i_flush has barriers; k2i_vec needs whole waves)
    for (uint64_t bv = (uint64_t)blockIdx.x * per_trip; bv < n_vec; bv += (uint64_t)gridDim.x * per_trip) {
        uint4 c[K2I_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < K2I_UNROLL; ++u) {
            const uint64_t vi = bv + (uint64_t)u * K2I_THREADS + tid;
            c[u] = vi < n_vec ? vec[vi] : make_uint4(0u, 0u, 0u, 0u);
        }
        uint32_t o = 0, b = 0;
#pragma unroll
        for (uint32_t u = 0; u < K2I_UNROLL; ++u) k2i_vec(c[u], lane, s_bins, a, o, b);
        occ += o; bad += b;
        if (++trips == K2I_FLUSH_TRIPS) { trips = 0; k2i_flush(s_bins, a); }      // bounds what a 32-bit bin can hold
    }
    if (blockIdx.x == 0 && tid < (uint32_t)(a.capacity & 3u)) {                   // the ragged end, cell by cell
        uint32_t o = 0, b = 0;
        const uint32_t v = k2i_value(a.cells[(n_vec << 2) + tid], a, o, b);
        occ += o; bad += b;
        if (v) k2i_add(s_bins, a, v, 1u);
    }
    k2i_flush(s_bins, a);
    if (a.ctr) {                                                                  // one add per wave and counter
        occ = wave_all_add_u64(occ); bad = wave_all_add_u64(bad);
        if (lane == 0 && occ) __hip_atomic_fetch_add(&a.ctr[0], occ, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 0 && bad) __hip_atomic_fetch_add(&a.ctr[1], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the two test switches, read per call: the grid, and the bin limit (0: every value takes the HBM adds)
static long k2i_switch(const char *name, long lo, long hi, long dflt)
{
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    const long v = atol(e);
    return v < lo ? lo : v > hi ? hi : v;
}

extern "C" sh_status sh_k2_value_counts_device(const sh_k2_db *db, uint64_t *d_counts, void *stream, sh_k2_inspect_stats *stats)
{
    SH_CHECK(db && d_counts, SH_ERR_BAD_ARG, "sh_k2_value_counts_device: null argument");
    const uint64_t n_nodes = db->nodes.size();
    SH_CHECK(db->value_bits >= 1 && db->value_bits <= 31 && n_nodes >= 1 && n_nodes <= (1ull << 31), SH_ERR_BAD_ARG,
             "sh_k2_value_counts_device: value_bits %d, %llu taxonomy nodes", db->value_bits, (unsigned long long)n_nodes);
    SH_HIP(hipSetDevice(db->device));
    hipStream_t s = (hipStream_t)stream;
    if (stats) { memset(stats, 0, sizeof(*stats)); stats->n_cells = db->capacity; }
    int n_cu = 0;
    SH_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, db->device));
    const uint64_t per_trip = (uint64_t)K2I_THREADS * K2I_UNROLL;
    const uint64_t n_trips = ((db->capacity >> 2) + per_trip - 1) / per_trip;
    uint32_t grid = (uint32_t)std::max<uint64_t>(std::min<uint64_t>((uint64_t)std::max(n_cu, 1) * K2I_BLOCKS_PER_CU, n_trips), 1);
    grid = (uint32_t)k2i_switch("SCRUBBY_HIP_K2_INSPECT_BLOCKS", 1, 1 << 20, (long)grid);
    const uint32_t limit = (uint32_t)k2i_switch("SCRUBBY_HIP_K2_INSPECT_LDS_BINS", 0, K2I_LDS_BINS_MAX, K2I_LDS_BINS);
    K2InspectArgs a{db->d_cells, db->capacity, (1u << db->value_bits) - 1u, (uint32_t)n_nodes, (uint32_t)std::min<uint64_t>(n_nodes, limit),
                    (unsigned long long *)d_counts, nullptr};
    SH_HIP(hipMemsetAsync(d_counts, 0, n_nodes * 8, s));
    if (!stats) {                                    // nothing to wait for: the call stays asynchronous on the stream
        hipLaunchKernelGGL(k_k2_value_counts, dim3(grid), dim3(K2I_THREADS), a.lds_bins * 4, s, a);
        SH_HIP(hipGetLastError());
        return SH_OK;
    }
    DevBuf b_ctr;
    DevEvent e0, e1;
    SH_HIP(b_ctr.alloc(16));
    SH_HIP(e0.create()); SH_HIP(e1.create());
    SH_HIP(hipMemsetAsync(b_ctr.p, 0, 16, s));
    a.ctr = b_ctr.as<unsigned long long>();
    SH_HIP(hipEventRecord(e0.e, s));
    hipLaunchKernelGGL(k_k2_value_counts, dim3(grid), dim3(K2I_THREADS), a.lds_bins * 4, s, a);
    SH_HIP(hipGetLastError());
    SH_HIP(hipEventRecord(e1.e, s));
    unsigned long long ctr[2] = {0, 0};
    SH_HIP(hipMemcpyAsync(ctr, b_ctr.p, 16, hipMemcpyDeviceToHost, s));
    SH_HIP(hipStreamSynchronize(s));
    stats->n_occupied = ctr[0]; stats->n_bad_values = ctr[1];
    SH_HIP(hipEventElapsedTime(&stats->ms, e0.e, e1.e));
    return SH_OK;
}

extern "C" sh_status sh_k2_value_counts(const sh_k2_db *db, uint64_t *counts, sh_k2_inspect_stats *stats)
{
    SH_CHECK(db && counts, SH_ERR_BAD_ARG, "sh_k2_value_counts: null argument");
    SH_HIP(hipSetDevice(db->device));
    const uint64_t n_nodes = db->nodes.size();
    DevBuf b_counts;
    SH_HIP(b_counts.alloc(std::max<uint64_t>(n_nodes, 1) * 8));
    sh_k2_inspect_stats local;
    sh_status st = sh_k2_value_counts_device(db, b_counts.as<uint64_t>(), nullptr, stats ? stats : &local);
    if (st == SH_OK && hipMemcpy(counts, b_counts.p, n_nodes * 8, hipMemcpyDeviceToHost) != hipSuccess) { sh_set_error("copy of the counts failed"); st = SH_ERR_HIP; }
    return st;
}

// ---- the reports (host only) -------------------------------------------------------------------------------------------------------
static const char *k2_pool(const std::string &pool, uint64_t off) { return off < pool.size() ? pool.c_str() + off : ""; }

// the letter of a rank that has one (upper case: the Kraken-style rank code; the MPA prefix is its lower case), or 0
static char k2_rank_letter(const std::string &rank)
{
    if (rank == "superkingdom") return 'D';
    if (rank == "kingdom") return 'K';
    if (rank == "phylum") return 'P';
    if (rank == "class") return 'C';
    if (rank == "order") return 'O';
    if (rank == "family") return 'F';
    if (rank == "genus") return 'G';
    if (rank == "species") return 'S';
    return 0;
}

void shi_k2_report_rows(FILE *f, const sh_k2_taxnode *nodes, size_t n, const std::string &names, const std::string &ranks, const uint64_t *clade,
                        const uint64_t *direct, double total, int32_t flags, const uint64_t *extra_a, const uint64_t *extra_b)
{
    const bool zero = (flags & SH_K2_INSPECT_ZERO_COUNTS) != 0, mpa = (flags & SH_K2_INSPECT_MPA) != 0;
    // depth-first from the root, children by clade count (descending; ties by id), rank codes with a depth suffix
    struct Frame { uint32_t id; std::string code; int code_depth; int depth; std::string path; };
    std::vector<Frame> stack;
    if (n > 1 && (clade[1] || zero)) stack.push_back(Frame{1, "R", 0, 0, ""});
    while (!stack.empty()) {
        Frame fr = stack.back(); stack.pop_back();
        const sh_k2_taxnode &nd = nodes[fr.id];
        std::string code = fr.code, path = fr.path; int cd = fr.code_depth;
        const char letter = k2_rank_letter(k2_pool(ranks, nd.rank_offset));
        if (fr.id != 1) {
            if (letter) { code = std::string(1, letter); cd = 0; } else ++cd;
        }
        if (mpa) {                   // the lettered ancestors and the taxon itself; a taxon without a letter is only descended through
            if (letter) {
                std::string name = k2_pool(names, nd.name_offset);
                std::replace(name.begin(), name.end(), ' ', '_');
                if (!path.empty()) path += '|';
                path += (char)(letter - 'A' + 'a'); path += "__"; path += name;
                fprintf(f, "%s\t%llu\n", path.c_str(), (unsigned long long)clade[fr.id]);
            }
        } else {
            std::string rc = code; if (cd) rc += std::to_string(cd);
            fprintf(f, "%6.2f\t%llu\t%llu\t", 100.0 * (double)clade[fr.id] / total, (unsigned long long)clade[fr.id], (unsigned long long)direct[fr.id]);
            if (extra_a && extra_b) fprintf(f, "%llu\t%llu\t", (unsigned long long)extra_a[fr.id], (unsigned long long)extra_b[fr.id]);
            fprintf(f, "%s\t%llu\t", rc.c_str(), (unsigned long long)nd.external_id);
            for (int i = 0; i < fr.depth; ++i) fputs("  ", f);
            fprintf(f, "%s\n", k2_pool(names, nd.name_offset));
        }
        std::vector<uint32_t> kids;
        for (uint64_t c = 0; c < nd.child_count; ++c) { const uint64_t id = nd.first_child + c; if (id < n && (clade[id] || zero)) kids.push_back((uint32_t)id); }
        std::sort(kids.begin(), kids.end(), [&](uint32_t x, uint32_t y) { return clade[x] != clade[y] ? clade[x] > clade[y] : x < y; });
        for (size_t i = kids.size(); i-- > 0;) stack.push_back(Frame{kids[i], code, cd, fr.depth + 1, path});
    }
}

extern "C" sh_status sh_k2_counts_report(const sh_k2_taxnode *nodes, uint64_t n_nodes, const char *names, uint64_t names_len, const char *ranks, uint64_t ranks_len,
                                         const uint64_t *counts, int32_t flags, const char *header, const char *path)
{
    SH_CHECK(nodes && counts && (names || names_len == 0) && (ranks || ranks_len == 0), SH_ERR_BAD_ARG, "sh_k2_counts_report: null argument");
    SH_CHECK(n_nodes >= 2, SH_ERR_BAD_ARG, "sh_k2_counts_report: a taxonomy has at least the empty node and the root");
    for (uint64_t i = 2; i < n_nodes; ++i)
        SH_CHECK(nodes[i].parent >= 1 && nodes[i].parent < i, SH_ERR_BAD_ARG, "sh_k2_counts_report: node %llu: ids must be breadth-first", (unsigned long long)i);
    const std::string name_pool(names ? names : "", names_len), rank_pool(ranks ? ranks : "", ranks_len);
    std::vector<uint64_t> direct(counts, counts + n_nodes), clade(counts, counts + n_nodes);
    direct[0] = clade[0] = 0;                                              // value 0 is no taxon
    uint64_t sum = 0;
    for (uint64_t i = 1; i < n_nodes; ++i) sum += direct[i];
    for (uint64_t i = n_nodes - 1; i >= 2; --i) clade[nodes[i].parent] += clade[i];      // parents have smaller ids
    const bool to_stdout = !path || strcmp(path, "-") == 0;
    FILE *f = to_stdout ? stdout : fopen(path, "w");
    SH_CHECK(f, SH_ERR_IO, "cannot write %s", path);
    if (header) fputs(header, f);
    shi_k2_report_rows(f, nodes, n_nodes, name_pool, rank_pool, clade.data(), direct.data(), sum ? (double)sum : 1.0, flags);
    const bool ok = to_stdout ? (fflush(f) == 0 && !ferror(f)) : (fclose(f) == 0);
    SH_CHECK(ok, SH_ERR_IO, "short write to %s", to_stdout ? "stdout" : path);
    return SH_OK;
}

static void k2_binary(std::string &o, uint64_t v, int digits)
{
    for (int b = digits - 1; b >= 0; --b) o += (char)('0' + ((v >> b) & 1u));
}

extern "C" sh_status sh_k2_inspect_header(const sh_k2_db *db, char *buf, uint64_t cap, uint64_t *len)
{
    SH_CHECK(db && (buf || cap == 0), SH_ERR_BAD_ARG, "sh_k2_inspect_header: null argument");
    // (kraken2-inspect as recalled: "protein db" for a protein database, whose l-mer has 4 bits a character)
    std::string o = std::string("# Database options: ") + (db->opts.protein ? "protein" : "nucleotide") + " db, k = " + std::to_string(db->opts.k) + ", l = " +
                    std::to_string(db->opts.l) + "\n# Spaced mask = ";
    k2_binary(o, db->opts.spaced_seed_mask, (db->opts.protein ? 4 : 2) * db->opts.l);
    o += "\n# Toggle mask = ";
    k2_binary(o, db->opts.toggle_mask, 64);
    o += "\n# Total taxonomy nodes: " + std::to_string(db->nodes.size()) + "\n# Table size: " + std::to_string(db->size) + "\n# Table capacity: " +
         std::to_string(db->capacity) + "\n# Min clear hash value = " + std::to_string(db->opts.min_acceptable_hash) + "\n";
    if (len) *len = o.size();
    if (cap) { const size_t m = std::min<size_t>(o.size(), (size_t)cap - 1); memcpy(buf, o.data(), m); buf[m] = 0; }
    return SH_OK;
}

// `scrubby-hip k2-inspect`
extern "C" sh_status sh_k2_inspect_run(const sh_k2_inspect_config *cfg, sh_k2_inspect_result *out)
{
    SH_CHECK(cfg && cfg->db, SH_ERR_BAD_ARG, "sh_k2_inspect_run: a database directory is required");
    using clk = std::chrono::steady_clock;
    auto secs = [](clk::time_point t0, clk::time_point t1) { return std::chrono::duration<double>(t1 - t0).count(); };
    sh_k2_inspect_result r{};
    const auto t0 = clk::now();
    sh_k2_db *db = nullptr;
    sh_status st = sh_k2_open(cfg->db, cfg->device, &db);
    if (st != SH_OK) return st;
    const auto t1 = clk::now();
    r.s_open = secs(t0, t1);
    r.capacity = db->capacity; r.size_header = db->size; r.n_nodes = db->nodes.size();
    auto body = [&]() -> sh_status {
        uint64_t hlen = 0;
        sh_k2_inspect_header(db, nullptr, 0, &hlen);
        std::string header(hlen + 1, '\0');
        sh_k2_inspect_header(db, &header[0], hlen + 1, nullptr);
        header.resize(hlen);
        const bool to_stdout = !cfg->output || strcmp(cfg->output, "-") == 0;
        if (cfg->skip_counts) {                      // the header only: nothing is launched
            const auto t2 = clk::now();
            FILE *f = to_stdout ? stdout : fopen(cfg->output, "w");
            SH_CHECK(f, SH_ERR_IO, "cannot write %s", cfg->output);
            fputs(header.c_str(), f);
            const bool ok = to_stdout ? (fflush(f) == 0 && !ferror(f)) : (fclose(f) == 0);
            SH_CHECK(ok, SH_ERR_IO, "short write to %s", to_stdout ? "stdout" : cfg->output);
            r.s_report = secs(t2, clk::now());
            return SH_OK;
        }
        std::vector<uint64_t> counts(db->nodes.size(), 0);
        sh_k2_inspect_stats stats{};
        const sh_status sc = sh_k2_value_counts(db, counts.data(), &stats);
        const auto t2 = clk::now();
        r.s_count = secs(t1, t2);
        if (sc != SH_OK) return sc;
        r.n_occupied = stats.n_occupied; r.n_bad_values = stats.n_bad_values;
        for (size_t i = 1; i < counts.size(); ++i) r.n_taxa_with_minimizers += counts[i] != 0;
        SH_CHECK(stats.n_bad_values == 0, SH_ERR_IO, "%s/hash.k2d: %llu occupied cells carry a value that is 0 or outside the taxonomy of %llu nodes", cfg->db,
                 (unsigned long long)stats.n_bad_values, (unsigned long long)db->nodes.size());
        if (stats.n_occupied != db->size)
            fprintf(stderr, "[scrubby-hip] %s/hash.k2d: the header says %llu cells are in use, the table holds %llu\n", cfg->db, (unsigned long long)db->size,
                    (unsigned long long)stats.n_occupied);
        const int32_t flags = (cfg->report_zero_counts ? SH_K2_INSPECT_ZERO_COUNTS : 0) | (cfg->use_mpa_style ? SH_K2_INSPECT_MPA : 0);
        const sh_status sr = sh_k2_counts_report(db->nodes.data(), db->nodes.size(), db->names.data(), db->names.size(), db->ranks.data(), db->ranks.size(),
                                                 counts.data(), flags, header.c_str(), cfg->output);
        r.s_report = secs(t2, clk::now());
        return sr;
    };
    st = body();
    sh_k2_free(db);
    r.s_total = secs(t0, clk::now());
    if (out) *out = r;
    return st;
}
