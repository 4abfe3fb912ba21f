// sh_host.h — declarations shared by the two host-side translation units (sh_host.cpp, sh_stream.cpp).
#pragma once
#include "sh_common.h"
#include <unordered_set>

struct ReportSettings {       // ScrubbySettings, /root/reference/src/report.rs:71-88 (field order = key order)
    const char *aligner = nullptr, *classifier = nullptr, *index = nullptr, *alignment = nullptr, *reads = nullptr, *report = nullptr, *preset_variant = nullptr;
    std::vector<std::string> taxa, taxa_direct;
    uint64_t min_len = 0; double min_cov = 0.0; uint32_t min_mapq = 0;
    bool extract = false;
    const char *classifier_args = nullptr;
};

// ScrubbyReport JSON (report.rs:10-88)
sh_status shi_write_report_json(const char *const *input, const char *const *output, uint32_t n_files, const char *command,
                                const ReportSettings &st, const sh_reads_result *r, const char *path);
// bzip2 / xz inputs (the reference reads them through niffler, utils.rs:377-383): recognised by their magic bytes and refused by name -
// this image ships libbz2 / liblzma without headers, so the backend links zlib only.  true = refused, error set.
bool shi_unsupported_compression(const char *path);
// -t <= 0: the CPUs this process may use (hardware threads, capped by the cgroup CPU quota and by 64)
int shi_default_threads();
// Preset's serde name ("Sr", "MapOnt", ...) from its Display form
const char *shi_preset_variant(const std::string &display);
// collect-then-map form of the whole path (sh_host.cpp)
sh_status shi_reads_run_legacy(const sh_reads_config *c, sh_reads_result *res);
// `scrubby reads -c kraken2`, collect-then-classify form (sh_host.cpp)
sh_status shi_kraken_run_legacy(const sh_kraken_config *c, sh_reads_result *res);
// get_taxids_from_report (/root/reference/src/classifier.rs:124-252)
sh_status shi_taxids_from_report(const char *report, const std::vector<std::string> &taxa_in, const std::vector<std::string> &direct_in,
                                 std::unordered_set<std::string> &out);
void shi_mkdir_p(const std::string &dir);
// `scrubby alignment` on a BAM file (sh_bam.hip): the names of the records the rule selects, added to ids.  The host path (zlib and
// sh_bam_filter_host) unless SCRUBBY_HIP_GUNZIP_DEVICE is 1 or 2 and device 0 is usable
sh_status shi_bam_ids(const char *path, uint64_t min_len, double min_cov, uint32_t min_mapq, std::unordered_set<std::string> &ids);
// column 5 of kraken.reads for one unit (sh_k2_format_hits), appended to o; false = a code outside the taxonomy
bool shi_k2_hitlist(std::string &o, const sh_k2_hit *e, uint64_t n, const uint32_t *external, uint64_t n_nodes, bool quick, uint32_t quick_taxid);
// the Kraken arm's classification of one host batch for both writers: the results and, unless opts.quick, every unit's hit list
struct ShiKrakenHits {
    bool quick = false;
    bool none = false;                  // a protein database: no hit lists, column 5 is "0:0"

    std::vector<uint64_t> off;          // n_units + 1
    std::vector<sh_k2_hit> ent;
    std::vector<uint32_t> ext;          // external ids of the taxonomy
    // column 5 of unit i (r: its result) appended to o
    void append(std::string &o, uint64_t i, const sh_k2_result &r) const
    {
        if (none) { o += "0:0"; return; }
        shi_k2_hitlist(o, quick ? nullptr : ent.data() + off[i], quick ? 0 : off[i + 1] - off[i], ext.data(), ext.size(), quick, r.taxid);
    }
};
// md (nullable): the run's minimizer-data accumulator (-C "--report-minimizer-data")
sh_status shi_kraken_classify(sh_k2_db *db, const sh_k2_opts &opts, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t n_rec,
                              bool paired, sh_k2_result *results, ShiKrakenHits &hits, sh_k2_mindata *md = nullptr);
// a protein database (DESIGN.md §7 "Translated search"): --quick and --report-minimizer-data are refused by name
sh_status shi_kraken_protein_checks(const sh_kraken_config *c, const sh_k2_opts &db_opts);
// kraken.minimizer.report beside kraken.report, when the run keeps an accumulator
sh_status shi_kraken_minimizer_report(const sh_kraken_config *c, sh_k2_db *db, const sh_k2_result *results, uint64_t n_units, sh_k2_mindata *md, const std::string &dir);
// database build: the <n> of a `kraken:taxid|<n>` sequence id (sh_host.cpp)
bool shi_k2_header_taxid(const char *id, size_t len, uint64_t *taxid);
// abundance re-estimation: the header -> taxon rule of sh_k2_taxonomy_header_taxon over the taxonomy a database already has (its
// nodes), with an id map (nullable) or one external taxid for every record (0: none).  A taxid the database lacks is named once on
// stderr; its sequences get no taxon.  Freed with sh_k2_taxonomy_free (sh_host.cpp)
sh_status shi_k2_taxonomy_of_nodes(const sh_k2_taxnode *nodes, uint64_t n_nodes, const char *seqid2taxid_map, uint64_t single_taxid, sh_k2_taxonomy **out);
