/*
 * scrubby_hip.h — C ABI of libscrubby_hip.so, the MI355X (gfx950) host-depletion backend.
 *
 * This is the drop-in boundary for the one hot path of esteinig/scrubby that this
 * library replaces: the in-process `mm2` aligner path
 *     Cleaner::run_minimap2_rs        /root/reference/src/cleaner.rs:443-575
 * whose arithmetic the reference reaches through the `minimap2` crate (FFI into
 * lh3/minimap2).  Every entry point below cites the reference interface it stands in
 * for; INTEGRATION.md shows the Rust `extern "C"` block a Scrubby maintainer would add.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns an sh_status (0 = OK) and
 *     never throws or aborts across the boundary; sh_last_error() gives the message
 *     (thread-local), mirroring the `&'static str` errors minimap2-rs hands to
 *     ScrubbyError::Minimap2RustAlignerBuilderFailed / Minimap2RustAlignmentFailed
 *     (/root/reference/src/error.rs:147-152).
 *   - the caller owns every input/output buffer; the library owns sh_index / sh_ctx.
 *   - "_device" variants take HIP device pointers (inputs already resident in HBM) and
 *     a hipStream_t passed as void*; the others take host pointers and stage through
 *     HBM internally.
 *   - a read batch is the reference's Vec<(id, Vec<u8>)> (cleaner.rs:547-549) flattened:
 *     `bases` = concatenated ASCII sequence bytes, `offsets[n_reads+1]` = start of each
 *     read in `bases`.  Paired-end input is simply two records per pair: the reference
 *     maps each mate independently as single-end (cleaner.rs:499-501,527-529).
 */
#ifndef SCRUBBY_HIP_H
#define SCRUBBY_HIP_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SH_VERSION 104   /* 0.1.3 (+ kraken2 --minimum-base-quality / --quick: fields appended to sh_k2_opts, sh_k2_stats, sh_kraken_config, classify entries that take qualities added; the old layouts are prefixes; + Kraken 2 hit lists: classify entries that return them, sh_k2_hits_*, sh_k2_format_hits added, nothing changed; + the eight older Kraken classify entries removed, the version kept: sh_k2_classify_ex_device / _batch is the one pair; + the Kraken arm's wave route: sh_k2_opts grew long_unit_bases, sh_k2_stats n_long_units / ms_long, the old layouts are prefixes, the version kept; + the Kraken arm's abundance re-estimation: sh_k2_distrib_*, sh_k2_bracken_* added, nothing changed, the version kept; + DEFLATE on the device: sh_deflate_*, sh_deflater_*, sh_gzip_member added, nothing changed, the version kept): sh_index_replicate / sh_classify_sharded, sh_ctx_debug_list 3..10, the long join's tree in LDS (round 5); 0.1.2: sh_stats grew n_locus_* / n_rmq_exact (round 4); 0.1.1: sh_opts grew the rmq_* fields (round 3); sh_trace has 12 words since 0.1.0's second round */

typedef int32_t sh_status;
enum {
    SH_OK = 0,
    SH_ERR_BAD_ARG = 1,        /* null pointer, unsupported k/w, ... */
    SH_ERR_PRESET_UNKNOWN = 2,
    SH_ERR_PRESET_UNSUPPORTED = 3, /* Preset::Lr -> ScrubbyError::Minimap2PresetNotSupported (cleaner.rs:469) */
    SH_ERR_NO_DEVICE = 4,
    SH_ERR_OOM = 5,
    SH_ERR_HIP = 6,
    SH_ERR_IO = 7,
    SH_ERR_EMPTY_READ = 8,     /* minimap2-rs: Err("Sequence is empty") -> Minimap2RustAlignmentFailed; aborts the run (cleaner.rs:552,566) */
    SH_ERR_INDEX = 9           /* index build failed -> Minimap2RustAlignerBuilderFailed (cleaner.rs:480-482) */
};

/* Mapping options = the subset of minimap2's mm_idxopt_t/mm_mapopt_t that decides
 * `mappings.len() > 0`; filled by sh_preset() the way Aligner::builder().sr() / .map_ont()
 * ... fill them (cleaner.rs:455-470).  Layout is shared with the device code. */
typedef struct sh_opts {
    int32_t k, w;
    int32_t is_sr;
    int32_t mid_occ;          /* <= 0: derived from the index (mm_mapopt_update) */
    int32_t max_occ;
    int32_t max_max_occ;
    int32_t occ_dist;
    int32_t min_mid_occ, max_mid_occ;
    float   mid_occ_frac;
    float   q_occ_frac;
    int32_t min_cnt, min_chain_score;
    int32_t max_gap, max_gap_ref, max_frag_len, bw;
    int32_t max_chain_skip, max_chain_iter;
    float   chain_gap_scale, chain_skip_scale;
    /* the base-level extension stage that `.with_cigar()` switches on (cleaner.rs:473): with
     * SH_F_CIGAR a read only counts as mapped when a region of one of its chains survives the banded alignment and
     * minimap2's mm_filter_regs (cnt >= min_cnt, mlen >= min_chain_score, dp_max >= min_dp_max).  sh_preset sets it. */
    int32_t flags;
    int32_t a, b, q, e, q2, e2, sc_ambi;          /* ksw2 scores: match, mismatch, gap open / extend (two affine pieces), N */
    int32_t zdrop, zdrop_inv, end_bonus, min_dp_max;
    int32_t best_n, bw_long, min_ksw_len;
    float   pri_ratio, mask_level, max_clip_ratio;
    /* long-read presets: minimap2 re-chains a read whose first chaining pass left more than one chain with mg_lchain_rmq
     * (mm_map_frag: bw_long > bw), unless the first chain is small on a short read (rmq_rescue_*) */
    int32_t rmq_inner_dist, rmq_size_cap, rmq_rescue_size;
    float   rmq_rescue_ratio;
} sh_opts;
#define SH_F_CIGAR 1
/* A/B and tests: k_expand writes the anchors of every repeat-path read to the arena and the sort kernels read them back, instead of
 * building them in the LDS sort buffer of the kernel that sorts them (late anchors).  Results do not depend on it. */
#define SH_F_NO_LATE_ANCHORS 2

/* Per-read decision trace (optional output; used by the parity tests). */
typedef struct sh_trace {
    int32_t n_mini, n_seed, n_anchor, rep_len, rechained, n_chain, best_score, flag;
    /* extension stage (0 without SH_F_CIGAR or without a chain): regions aligned, regions left (= mappings.len()),
     * their largest dp_max, a fingerprint of their coordinates / mlen / blen / dp_max / cnt */
    int32_t n_aligned, n_regs, dp_max; uint32_t sig;
} sh_trace;

typedef struct sh_index_info {
    int32_t  k, w;
    int32_t  mid_occ;          /* resolved value (sr: 1000; map-ont: from index) */
    uint32_t n_contigs;
    uint64_t n_bases;
    uint64_t n_minimizers;     /* stored (hash,pos) pairs */
    uint64_t n_keys;           /* distinct minimizer hashes */
    uint64_t n_slots;          /* 16-B table slots */
    uint64_t n_positions;      /* entries of the multi-occurrence position array */
    uint64_t hbm_bytes;        /* table + positions resident in HBM */
    double   build_ms;
} sh_index_info;

typedef struct sh_stats {
    uint64_t n_reads;
    uint64_t n_host;           /* flags == 1 */
    uint64_t n_no_seed;        /* decided by the sketch/probe kernel alone */
    uint64_t n_chain_small;    /* reads chained in LDS (lane per read) */
    uint64_t n_chain_large;    /* reads chained in the HBM arena */
    uint64_t n_minimizers;     /* sum of sketch sizes = table probes issued */
    uint64_t n_bases;
    double   ms_sketch_probe;  /* HIP-event time of each stage, summed over chunks */
    double   ms_chain_small;
    double   ms_chain_large;
    double   ms_total;         /* first kernel start -> last kernel end */
    uint64_t n_anchors;        /* anchors the occurrence filter admits on the repeat path (both passes); flag-only calls generate fewer (n_pair_decided) */
    uint64_t n_clusters;       /* independent anchor clusters chained on the repeat path */
    uint64_t n_resketch;       /* reads that took the legacy re-sketch path */
    uint64_t n_pair_decided;   /* flag-only calls: reads (LDS path and repeat path) decided by two co-diagonal seeds, before any anchor exists */
    uint64_t n_ext_reads;      /* SH_F_CIGAR: reads whose chains went through the extension stage (not decided by a shortcut) */
    uint64_t n_ext_regions;    /* regions aligned for them */
    uint64_t n_ext_dropped;    /* reads with a chain but no surviving region: the flags this stage flips */
    double   ms_ext;           /* HIP-event time of the extension stage */
    uint64_t n_ext_shortcut;   /* SH_F_CIGAR flag-only: reads decided inside a chaining kernel - their top chain's max stretch alone passes mm_filter_regs */
    uint64_t n_ext_fallback;   /* SH_F_CIGAR flag-only, sr: reads whose regs[0] did not survive and that were re-chained with every chain kept */
    double   ms_ext_fallback;  /* wall time of that fallback (re-chaining + the complete procedure) */
    uint64_t n_ext_unresolved; /* reads the extension stage left at their chain-level answer, mapped (see the warning): the device had no memory left for them, or - long reads - the long join's inner window (1000 reference bases) outgrew the 4096-anchor LDS ring (chained exactly, at seconds per read, with SCRUBBY_HIP_RMQ_ONE_LANE=1) */
    uint64_t n_rmq_rechained;  /* long-read presets: reads re-chained by the RMQ long join */
    uint64_t n_rmq_tied;       /* ... of which met candidates of equal priority in the join in a way that can change the chains (ties that cannot are recognised and pass) */
    uint64_t n_dp_parallel;    /* repeat-path reads whose mg_lchain_dp ran as the parallel recurrence */
    uint64_t n_dp_dirty;       /* ... their anchors that broke its premise (their clusters were chained by the sequential code) */
    uint64_t n_top_settled;    /* ... reads whose candidates for regs[0] were read off the whole read, no cluster visited */
    uint64_t n_locus_reads;    /* long-read presets, flag-only: reads chained over the reference windows that can hold regs[0] only */
    uint64_t n_locus_redone;   /* ... of which the answer could depend on what was left out: redone with every anchor */
    uint64_t n_rmq_exact;      /* long-read presets: reads whose RMQ join was redone on the literal krmq tree (tied priorities, windows beyond the LDS ring, rmq_size_cap) */
    uint64_t n_rmq_open;       /* ... reads that met such a tie and kept the scan's choice (smallest index): 0 by default since round 5 (every tied read takes the tree); only with SCRUBBY_HIP_RMQ_EXACT_MAX = N >= 0, for reads of more than N chain anchors */
    uint64_t n_ext_ondemand;   /* reads beyond the extension stage's prepared working-memory sizes, redone with memory allocated for them (visits, both kernels) */
    uint64_t n_lc_filtered;    /* SH_F_CIGAR flag-only, counted with SCRUBBY_HIP_DBG & 16 only: reads k_local_cluster decided although a seed of theirs lies above mid_occ (part of n_ext_shortcut) */
    uint64_t n_late_reads;     /* table entries of the sort classes whose anchors the sort kernels build themselves (late anchors; 0 with SH_F_NO_LATE_ANCHORS) */
    uint64_t n_deferred;       /* times a repeat-path read found no arena room and was put off to the pass's next iteration */
} sh_stats;

typedef struct sh_index sh_index;
typedef struct sh_ctx sh_ctx;

/* ---- library ------------------------------------------------------------------------ */
int32_t     sh_version(void);
int32_t     sh_device_count(void);
const char *sh_last_error(void);

/* Aligner::builder().<preset>()  (cleaner.rs:453-470); name = Preset's Display form
 * ("sr", "map-ont", "lr:hq", ...; /root/reference/src/scrubby.rs:137-155). */
sh_status sh_preset(const char *name, sh_opts *out);

/* ---- index:  .with_index_threads(t).with_index(path, None)  (cleaner.rs:472-482) ----- */
/* Build from host sequences (already parsed FASTA records). */
sh_status sh_index_build(const uint8_t *const *seqs, const uint64_t *lens, uint32_t n_seq,
                         const sh_opts *opts, int32_t device, sh_index **out);
/* Build from a reference already resident in HBM: `d_bases` = concatenated ASCII contigs,
 * `contig_starts[n_contigs+1]` (host array) = start of each contig in d_bases. */
sh_status sh_index_build_device(const uint8_t *d_bases, const uint64_t *contig_starts, uint32_t n_contigs,
                                const sh_opts *opts, int32_t device, void *stream, sh_index **out);
/* Build from a FASTA file (plain or gzip); the reference rebuilds the index from FASTA on
 * every run (cleaner.rs:475-479). */
sh_status sh_index_build_fasta(const char *path, const sh_opts *opts, int32_t device, sh_index **out);
/* Binary cache of a built index (the reference passes output=None). */
sh_status sh_index_save(const sh_index *idx, const char *path);
sh_status sh_index_load(const char *path, int32_t device, sh_index **out);
sh_status sh_index_info_get(const sh_index *idx, sh_index_info *out);
/* Copy table and position array to host (tests, CPU baseline).  Either pointer may be NULL. */
sh_status sh_index_export(const sh_index *idx, uint64_t *slots /* 2*n_slots */, uint64_t *positions);
/* The reference bases the extension stage aligns against (minimap2 keeps them in the index too: mi->S), as resident in HBM:
 * 4-bit nt4 codes (A C G T = 0..3, anything else 4), two per byte, low nibble = even position, contigs back to back;
 * packed[(n_bases + 1) / 2], contig_start[n_contigs + 1].  Either pointer may be NULL. */
sh_status sh_index_export_ref(const sh_index *idx, uint8_t *packed, uint64_t *contig_start);
sh_status sh_index_free(sh_index *idx);

/* ---- classification:  aligner.map(&seq,false,false,None,None) -> len()>0  (cleaner.rs:550-558) --- */
/* A context owns the stream-ordered scratch (seed records, work lists, chain arena) for
 * batches of up to max_reads reads / max_bases bases; it plays the role of minimap2's
 * thread-local mm_tbuf_t.  One context per host thread; contexts share the immutable index. */
sh_status sh_ctx_create(const sh_index *idx, const sh_opts *opts, uint64_t max_reads, uint64_t max_bases,
                        uint32_t max_read_len, sh_ctx **out);
sh_status sh_ctx_destroy(sh_ctx *ctx);
/* Measurement aid (bench.py's stratified parity sample): which reads the context classified took the rarer paths.
 * Short-read extension stage, reads of the LAST CHUNK (ordinals within it): which = 0: re-chained with max_occ (mm_map_frag's second
 * pass), 1: regs[0] aligned base by base, 2: the complete procedure over every chain.
 * Long-read extension stage, reads of the LAST CALL (ordinals within it): which = 3: long join redone with the literal krmq tree beside the
 * scan (a tie that matters, or a window beyond the first ring), 4: tie left open (only with SCRUBBY_HIP_RMQ_EXACT_MAX >= 0), 5: left at the
 * chain-level answer (sh_stats.n_ext_unresolved), 6: redone with every anchor after the locus selection, 7: working memory allocated on
 * demand, 8: probe undecided - the complete procedure answered, 9: second working-memory size, 10: long join on the one-lane trees.
 * *n_out = their number (out may be NULL). */
sh_status sh_ctx_debug_list(const sh_ctx *ctx, int32_t which, uint32_t *out, uint64_t cap, uint64_t *n_out);

/* Inputs and outputs in HBM.  d_flags[r] = 1 host (>=1 mapping), 0 retained, 2 empty read.
 * d_trace may be NULL.  Asynchronous on `stream`; stats (nullable) forces a stream sync. */
sh_status sh_classify_device(sh_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                             uint64_t n_bases, uint8_t *d_flags, sh_trace *d_trace, void *stream, sh_stats *stats);

/* Host buffers in, host flags out.  The batch goes up in pieces of 4 Mi reads from the calling thread while a worker
 * thread classifies the pieces that have arrived (20 M x 150 bp from pageable memory: 0.29 s with the extension filter on, 0.08 s at chain level, PCIe included).  The
 * context, device buffers and streams a call needs stay with the index for the next call (any thread; concurrent calls
 * each get their own set) and are released by sh_index_free.
 * Returns SH_ERR_EMPTY_READ (after filling flags) if any read is empty, as the reference's
 * per-read Err aborts the run. */
sh_status sh_classify_batch(const sh_index *idx, const sh_opts *opts, const uint8_t *bases, const uint64_t *offsets,
                            uint64_t n_reads, uint8_t *out_flags, sh_trace *out_trace, sh_stats *stats);

/* ---- in-process multi-GPU (SURVEY.md 8(b) "Threading", 8(e)) -------------------------------------------------------
 * The reference shares ONE &Aligner among all rayon workers (cleaner.rs:546-559).  A set holds one replica of the index per
 * shard: devices[i] is shard i's device (NULL / 0: every visible device, one shard each; a device may be listed more than
 * once - logical shards); the source index is borrowed for its own device (free the set first), the other devices get
 * copies (device to device where the devices are peers), freed with the set. */
typedef struct sh_index_set sh_index_set;
sh_status sh_index_replicate(const sh_index *idx, const int32_t *devices, uint32_t n_devices, sh_index_set **out);
uint32_t  sh_index_set_size(const sh_index_set *set);
sh_status sh_index_set_free(sh_index_set *set);
/* sh_classify_batch over all replicas at once: the batch is cut into contiguous shards at even record ordinals (mates stay
 * together), balanced by bases (= by count for fixed-length records); each shard is classified on its device by a host thread
 * of its own; the flags land in the caller's array - disjoint ranges, so the union of cleaner.rs:564-570 is a concatenation
 * and needs no collective.  shard_first (nullable, n_shards + 1 entries) receives the first record of each shard.  stats:
 * counters summed, stage times the largest over the devices.  Errors as sh_classify_batch; the message names the shard. */
sh_status sh_classify_sharded(const sh_index_set *set, const sh_opts *opts, const uint8_t *bases, const uint64_t *offsets,
                              uint64_t n_reads, uint8_t *out_flags, sh_trace *out_trace, sh_stats *stats, uint64_t *shard_first);

/* ---- the whole replaced path:  Cleaner::run_minimap2_rs + clean_reads + ScrubbyReport  ------------------------
 * (/root/reference/src/cleaner.rs:443-575, :236-254, :731-760; src/report.rs:24-57; src/utils.rs:250-285)
 * FASTA/FASTQ (plain, gzip, bzip2 or xz: sniffed by magic bytes like needletail / niffler do) in, filtered files out (the container by the
 * output's extension: utils.rs:28-36), optional JSON report and TSV of removed ids.
 * This is what `scrubby reads -i R1 [R2] -o O1 [O2] -I ref.fa [-p sr] [-e] [-j report.json] [-r ids.tsv]` runs. */
typedef struct sh_reads_config {
    const char *input[2];
    const char *output[2];
    uint32_t    n_files;      /* 1 (single-end / long reads) or 2 (paired-end) */
    int32_t     extract;      /* -e: write the mapped reads instead of the unmapped ones */
    const char *index;        /* -I: reference FASTA(.gz), or a .shidx cache written by sh_index_save */
    const char *preset;       /* -p: NULL -> "sr" for two files, "map-ont" for one (scrubby.rs:935-951) */
    const char *json;         /* -j, nullable */
    const char *read_ids;     /* -r, nullable */
    const char *command;      /* argv joined by ' ' (terminal.rs:178), for the report */
    int32_t     threads;      /* -t: host threads of the parse / filter / deflate stages (> 0: as given; <= 0: the CPUs this process may use - hardware threads capped by the cgroup quota and by 64) */
    int32_t     device;
} sh_reads_config;

typedef struct sh_reads_result {
    uint64_t reads_in, reads_out, reads_removed, reads_extracted;   /* as in the JSON report (records over both files) */
    uint64_t n_depleted_ids;                                        /* size of the HashSet<String> of cleaner.rs:564-570 */
    double   ms_index, ms_ingest, ms_classify, ms_write;
    uint64_t n_ext_unresolved;   /* reads the extension stage left at their chain-level answer (mapped); sh_stats of the same name, summed over the run's calls */
    uint64_t n_rmq_open;         /* long reads whose long join met a tie that matters beyond SCRUBBY_HIP_RMQ_EXACT_MAX anchors (sh_stats.n_rmq_open) */
} sh_reads_result;

sh_status sh_reads_run(const sh_reads_config *cfg, sh_reads_result *out);
/* sh_reads_run / sh_kraken_run keep the classification context of the last run (tens of GB of HBM scratch) for the next run of the
 * process, because handing such memory back and asking for it again costs seconds (the driver wipes it).  A long-lived embedding
 * process gets that memory back with this call; SCRUBBY_HIP_CTX_CACHE=0 in the environment switches the caching off.  Returns SH_OK. */
sh_status sh_release_cached_ctx(void);

/* ---- `scrubby classifier`: cleaning from precomputed Kraken2 / Metabuli outputs ------------------------------------
 * Cleaner::run_classifier_output (cleaner.rs:177-194) with the taxid decision rule of src/classifier.rs:
 * get_taxids_from_report (:124-252), get_tax_level (:345-373), get_taxid_reads_kraken / _metabuli (:270-320).
 * String / integer logic only: no GPU involved. */
typedef struct sh_classifier_config {
    const char *input[2];
    const char *output[2];
    uint32_t    n_files;
    int32_t     extract;
    const char *report;             /* -k: Kraken-style report */
    const char *reads;              /* -j: per-read classifications */
    const char *classifier;         /* -c: "kraken2" | "metabuli" */
    const char *const *taxa;        /* -T: names or taxids; sub-levels with direct reads are included */
    uint32_t    n_taxa;
    const char *const *taxa_direct; /* -D: names or taxids taken as they are */
    uint32_t    n_taxa_direct;
    const char *json;               /* --json, nullable */
    const char *read_ids;           /* -r, nullable */
    const char *command;
} sh_classifier_config;

sh_status sh_classifier_run(const sh_classifier_config *cfg, sh_reads_result *out);
/* the taxid set alone: sorted, newline-separated into `out` */
sh_status sh_classifier_taxids(const char *report, const char *const *taxa, uint32_t n_taxa, const char *const *taxa_direct,
                               uint32_t n_direct, char *out, size_t cap, uint64_t *n_out);

/* ---- `scrubby alignment`: cleaning from a precomputed alignment (PAF/GAF, SAM/BAM, or a one-column TXT of read ids) ---------
 * Cleaner::run_aligner_output (cleaner.rs:206-219), ReadAlignment::from / from_paf / from_txt / from_bam (alignment.rs:33-211):
 * a read is selected iff (query aligned length >= min_len OR query coverage >= min_cov) AND mapq >= min_mapq.
 * SAM and BAM (the reference's optional htslib feature) are read here: within the two formats the content decides, a gzip stream
 * whose first inflated bytes are "BAM\1" is BAM, anything else is SAM text (sh_bam_* below).  CRAM is rejected by name. */
typedef struct sh_alignment_config {
    const char *input[2];
    const char *output[2];
    uint32_t    n_files;
    int32_t     extract;
    const char *alignment;    /* -a */
    const char *format;       /* "paf" | "gaf" | "txt" | "sam" | "bam", or NULL: by the file's (last) extension */
    uint64_t    min_len;      /* -l */
    double      min_cov;      /* -c */
    uint32_t    min_mapq;     /* -q */
    const char *json, *read_ids, *command;
} sh_alignment_config;

sh_status sh_alignment_run(const sh_alignment_config *cfg, sh_reads_result *out);

/* host-side pieces on their own (no GPU needed): get_id (utils.rs:91-103), FastqCleaner::clean_reads
 * (cleaner.rs:731-760), ReadDifference::get_difference (utils.rs:250-285) */
sh_status sh_host_get_id(const char *header, char *out, size_t cap);
sh_status sh_host_filter_fastx(const char *in, const char *out, const char *const *ids, uint64_t n_ids, int32_t extract,
                               uint64_t *n_in, uint64_t *n_out);
sh_status sh_host_read_difference(const char *const *inputs, const char *const *outputs, uint32_t n, uint64_t *reads_in,
                                  uint64_t *reads_out, uint64_t *difference);
/* the chunked, multi-threaded form of the same filter that sh_reads_run uses (pass 2 of csrc/sh_stream.cpp): the input is cut
 * into chunks of ~chunk_bytes at record boundaries, `threads` workers filter (and deflate, for .gz outputs), one writer
 * write side by side; retain: 0 = stream the file, 1 = keep the parsed chunks of the sequential reader, 2 = of the boundary-guessing
 * reader, 3 = of several byte-range readers (pass 1's forms).  Same bytes out as
 * sh_host_filter_fastx for plain outputs; .gz outputs are multi-member gzip with the same decompressed content. */
sh_status sh_host_filter_fastx_stream(const char *in, const char *out, const char *const *ids, uint64_t n_ids, int32_t extract,
                                      uint64_t chunk_bytes, int32_t threads, int32_t retain, uint64_t *n_in, uint64_t *n_out);

/* ---- synthetic workload (bench/test utility) ---------------------------- */
/* params structs are syn_ref_params / syn_read_params of csrc/sh_synth_core.h, passed opaquely */
sh_status sh_synth_ref_device(const void *ref_params, uint64_t g0, uint64_t n, uint8_t *d_out, void *stream);
sh_status sh_synth_reads_device(const void *ref_params, const void *read_params, uint64_t r0, uint64_t n_records,
                                uint8_t *d_out, uint64_t *d_offsets /* n_records+1, may be NULL */, void *stream);

/* variable-length long reads (BASELINE config 4 stand-in); d_offsets[n_records+1] given by the caller (lengths: syn_long_len) */
sh_status sh_synth_long_reads_device(const void *ref_params, const void *read_params, uint64_t r0, uint64_t n_records,
                                     const uint64_t *d_offsets, uint64_t n_bases, uint8_t *d_out, void *stream);

/* ---- Kraken2-style taxid classifier (BASELINE configs[4]) ------------------------
 * Replaces the external process of Cleaner::run_kraken (/root/reference/src/cleaner.rs:288-330):
 *     kraken2 --threads T --db DB [--paired] IN.. --output kraken.reads --report kraken.report
 * The database (compact hash table of 32-bit cells + taxonomy) is resident in HBM; reads are scanned for (k, l)
 * minimizers, each distinct consecutive minimizer is probed once, every k-mer counts for its minimizer's taxon and the
 * call is Kraken2's ResolveTree.  File formats of a database directory: hash.k2d, opts.k2d, taxo.k2d. */
typedef struct sh_k2_db sh_k2_db;

typedef struct sh_k2_opts {
    int32_t  k, l;                  /* 35, 31 */
    uint64_t spaced_seed_mask;      /* --minimizer-spaces 7 */
    uint64_t toggle_mask;           /* 0xe37e28c4271b5a2d */
    uint64_t min_acceptable_hash;   /* down-sampled databases ("standard-8"): minimizers hashing below it are not looked up */
    int32_t  value_bits;            /* low bits of a cell = internal taxid (set from hash.k2d on open) */
    int32_t  min_hit_groups;        /* --minimum-hit-groups, default 2 */
    double   confidence;            /* --confidence, default 0 (a double, as Kraken 2 parses it: ceil(c * kmers) decides) */
    int32_t  min_base_quality;      /* --minimum-base-quality, default 0: a base whose Phred score is below it is ambiguous ('x');
                                       needs the qualities of the _q entries */
    int32_t  quick;                 /* --quick, default 0: the call is the first hit once min_hit_groups are seen, no ResolveTree
                                       (unclassified when no k-mer gets there); total_kmers counts the k-mers before that hit */
    int32_t  long_unit_bases;       /* a unit whose longer fragment has at least this many bases is classified by one wave
                                       (k_k2_classify_wave) instead of one lane; 0 = the default (DESIGN.md §7 "Long reads"),
                                       negative = never.  The answers do not depend on it; --quick units never take that route */
    int32_t  protein;               /* 1: the database holds amino-acid minimizers and reads are searched in six translated frames
                                       (DESIGN.md §7 "Translated search"); 0: nucleotides.  Set from opts.k2d on open; a call whose
                                       value disagrees with the database is SH_ERR_BAD_ARG */
} sh_k2_opts;

typedef struct sh_k2_taxnode {      /* taxo.k2d node: 7 x u64 */
    uint64_t parent, first_child, child_count, name_offset, rank_offset, external_id, godparent;
} sh_k2_taxnode;

typedef struct sh_k2_result {
    uint32_t taxid;         /* external (NCBI) taxid of the call, 0 = unclassified */
    uint32_t call;          /* internal taxid */
    uint32_t total_kmers;   /* k-mers of the read / pair (ambiguous ones included) */
    uint32_t hit_groups;    /* distinct consecutive minimizers found in the table */
} sh_k2_result;

typedef struct sh_k2_info {
    uint64_t capacity, size, n_nodes, hbm_bytes;
    int32_t  k, l, value_bits, key_bits;
} sh_k2_info;

typedef struct sh_k2_stats {
    uint64_t n_units, n_classified, n_probes, n_kmers, n_overflow;
    float    ms_classify, ms_total;
    uint64_t n_masked_bases;        /* bases of the batch masked by min_base_quality */
    uint64_t n_long_units;          /* units classified one wave per unit (opts.long_unit_bases) */
    float    ms_long;               /* that kernel's share of ms_classify */
    float    ms_translate;          /* protein databases: the six-frame translation of the batch (k_k2_translate), not in ms_classify */
} sh_k2_stats;

sh_status sh_k2_default_opts(sh_k2_opts *out);
/* the same for a protein database: k 15, l 12 (amino acids), no spaced seed, the same toggle mask, protein 1 */
sh_status sh_k2_default_protein_opts(sh_k2_opts *out);
/* Six-frame translation (DESIGN.md §7 "Translated search"; aa_translate.cc as recalled: PARITY UNPINNED).  Record r of n bases
 * gives frames 0..5 of (n-1)/3, (n-2)/3, n/3 residues forward and as many reverse (none for n < 3): the codon that ends at base i
 * is residue (i-2)/3 of forward frame i % 3, and its reverse complement residue n_f-1-(i-2)/3 of frame 3 + i % 3; a codon with a
 * base outside ACGTacgt, or one whose quality is below min_qual (quals nullable, byte 0xFF never masked), is X.  The frames are
 * written back to back in frame order from out[2 * (offsets[r] - offsets[0])]; out holds 2 * n_bases + 8 bytes, the bytes
 * between records are not written.  An output byte is the amino-acid scanner's code 0..15 (0x80: ambiguous, X), or with
 * as_letters != 0 the residue itself (A..Y, *, X).  _device: device pointers, work on `stream`, one synchronisation (the batch's
 * extent is read back before the launch; the kernel itself is only enqueued).
 * _host: the same on the CPU (no GPU needed). */
sh_status sh_k2_translate_device(const uint8_t *d_bases, const uint8_t *d_quals, const uint64_t *d_offsets, uint64_t n_records, int32_t min_qual,
                                 int32_t as_letters, uint8_t *d_out, void *stream);
sh_status sh_k2_translate_host(const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t n_records, int32_t min_qual,
                               int32_t as_letters, uint8_t *out);
/* k-mers per tile of the wave route (a fragment with more of them is scanned in several tiles) */
uint32_t sh_k2_wave_tile(void);
/* open a Kraken2 database directory (hash.k2d, opts.k2d, taxo.k2d) into HBM */
sh_status sh_k2_open(const char *dbdir, int device, sh_k2_db **out);
/* an empty table of `capacity` cells over a caller-supplied taxonomy (synthetic databases, tests).  Node 0 is the
 * unused sentinel, node 1 the root; parents precede children (breadth-first ids). */
sh_status sh_k2_create(const sh_k2_opts *opts, uint64_t capacity, const sh_k2_taxnode *nodes, uint64_t n_nodes,
                       const char *names, uint64_t names_len, const char *ranks, uint64_t ranks_len, int device, sh_k2_db **out);
/* insert (minimizer, internal taxid) pairs that are resident in HBM; a key already present keeps the LCA */
sh_status sh_k2_insert_device(sh_k2_db *db, const uint64_t *d_keys, const uint32_t *d_taxa, uint64_t n, void *stream);
/* insert every minimizer of a device-resident sequence [d_bases, d_bases + n) with one taxid (down-sampled by
 * opts.min_acceptable_hash); *n_inserted (nullable) receives the number of minimizer runs inserted */
sh_status sh_k2_insert_sequence_device(sh_k2_db *db, const uint8_t *d_bases, uint64_t n, uint32_t taxon, void *stream, uint64_t *n_inserted);
/* pseudo-random filler keys (synthetic databases): n keys derived from `seed`, taxa uniform in [taxon_lo, taxon_hi] */
sh_status sh_k2_insert_random(sh_k2_db *db, uint64_t seed, uint64_t n, uint32_t taxon_lo, uint32_t taxon_hi, void *stream);
sh_status sh_k2_save(const sh_k2_db *db, const char *dbdir);
sh_status sh_k2_info_get(const sh_k2_db *db, sh_k2_info *out);
/* the option set stored with the database (k, l, masks, down-sampling threshold) plus the default thresholds */
sh_status sh_k2_db_opts(const sh_k2_db *db, sh_k2_opts *out);
/* host copies for the test oracle: cells[capacity], parent[n_nodes], external[n_nodes] (any pointer may be NULL) */
sh_status sh_k2_export(const sh_k2_db *db, uint32_t *cells, uint32_t *parent, uint32_t *external);
sh_status sh_k2_free(sh_k2_db *db);
/* Kraken 2's per-k-mer hit list (column 5 of its output): per unit, in read order, the run-length encoding of the k-mers'
 * taxa.  code = internal taxid (0: not in the table, or not looked up in a down-sampled database), SH_K2_HIT_AMBIGUOUS
 * (ambiguous k-mers, masked bases included) or SH_K2_HIT_BORDER (the mate border of a pair, count 0, never merged).
 * Adjacent runs of one code merge; the counts without the border add up to the unit's total_kmers. */
#define SH_K2_HIT_AMBIGUOUS 0xFFFFFFFFu
#define SH_K2_HIT_BORDER    0xFFFFFFFEu
typedef struct sh_k2_hit { uint32_t code, count; } sh_k2_hit;
typedef struct sh_k2_hits sh_k2_hits;   /* the lists of one classify call (below), in HBM; freed with sh_k2_hits_free */
/* units, entries, and units whose lists were redone by the overflow pass (any pointer may be NULL) */
sh_status sh_k2_hits_count(const sh_k2_hits *hits, uint64_t *n_units, uint64_t *n_entries, uint64_t *n_redone);
/* unit i's entries are [offsets[i], offsets[i + 1]); device pointers owned by the handle, or host copies (offsets: n_units + 1,
 * entries: n_entries) */
sh_status sh_k2_hits_device(const sh_k2_hits *hits, const uint64_t **d_offsets, const sh_k2_hit **d_entries);
sh_status sh_k2_hits_copy(const sh_k2_hits *hits, uint64_t *offsets, sh_k2_hit *entries);
sh_status sh_k2_hits_free(sh_k2_hits *hits);
/* host only: column 5 of kraken.reads for one unit: "<taxid>:<n>", "A:<n>", "|:|" separated by single spaces (external ids
 * from external[n_nodes]); "0:0" for a unit without entries; with quick != 0, "<quick_taxid>:Q" whatever the entries.
 * Writes at most cap bytes including the terminating NUL; *len (nullable) = the full length without it.  A code outside the
 * taxonomy is SH_ERR_BAD_ARG. */
sh_status sh_k2_format_hits(const sh_k2_hit *entries, uint64_t n_entries, const uint32_t *external, uint64_t n_nodes, int32_t quick,
                            uint32_t quick_taxid, char *buf, uint64_t cap, uint64_t *len);
/* Kraken-style report (pct, clade reads, direct reads, rank code, taxid, indented name) from per-unit calls */
sh_status sh_k2_write_report(const sh_k2_db *db, const sh_k2_result *results, uint64_t n_units, const char *path);

/* ---- minimizer data (kraken2 --report-minimizer-data; DESIGN.md §7 "Minimizer data"; PARITY UNPINNED) ------------------------
 * Per taxon: n_minimizers, the lookups that returned it (exactly the ones that count as hit groups, whatever the unit's call),
 * and a dense HyperLogLog sketch (precision 12: 4096 one-byte registers) of the minimizers looked up.  The clade values are the
 * sum and the element-wise register maximum over the subtree.  sh_k2_mindata is the accumulator of one database in HBM
 * (n_nodes * 4096 B of registers and n_nodes counters; the first read-out allocates as much again for the clade values);
 * classify calls add to it, in any batching: counts add, registers merge by maximum. */
typedef struct sh_k2_mindata sh_k2_mindata;
sh_status sh_k2_mindata_create(const sh_k2_db *db, sh_k2_mindata **out);      /* SH_ERR_OOM names the size */
sh_status sh_k2_mindata_reset(sh_k2_mindata *md);
sh_status sh_k2_mindata_free(sh_k2_mindata *md);
/* The classify entries: _device takes device-resident records (device pointers in the batch, results to d_out, work on `stream`),
 * _batch the same from host memory (host pointers, results to out).
 *   batch   paired != 0: records 2i and 2i+1 are the mates of pair i (n_records even, else SH_ERR_BAD_ARG), one result per pair;
 *           else one result per record.  Device form: bases needs 8 readable bytes past the last base.
 *           quals (nullable: nothing is masked) holds Phred qualities for opts->min_base_quality, one byte per base at the
 *           offsets of bases, 0xFF = never masked (FASTA records).  Device form: quals and bases at the same address modulo 8
 *           (else SH_ERR_BAD_ARG) and 8 readable bytes past the last quality.
 *   hits    nullable; else *hits receives Kraken 2's hit lists (above) behind a handle the caller frees; results and stats are
 *           bit-identical to a call without them.  With opts->quick SH_ERR_BAD_ARG.  *hits is NULL after any failure.
 *   md      nullable; else the minimizer data of this database (else SH_ERR_BAD_ARG), which the call accumulates into;
 *           results and stats are bit-identical to a call without it. */
typedef struct sh_k2_batch {
    const uint8_t  *bases;
    const uint8_t  *quals;
    const uint64_t *offsets;
    uint64_t        n_records;
    int32_t         paired;
} sh_k2_batch;
sh_status sh_k2_classify_ex_device(const sh_k2_db *db, const sh_k2_opts *opts, const sh_k2_batch *batch, sh_k2_result *d_out, void *stream,
                                   sh_k2_stats *stats, sh_k2_hits **hits, sh_k2_mindata *md);
sh_status sh_k2_classify_ex_batch(const sh_k2_db *db, const sh_k2_opts *opts, const sh_k2_batch *batch, sh_k2_result *out, sh_k2_stats *stats,
                                  sh_k2_hits **hits, sh_k2_mindata *md);
/* per internal taxon (n_nodes each, any pointer may be NULL): own and clade lookup counts, own and clade distinct estimates */
sh_status sh_k2_mindata_counts(sh_k2_mindata *md, uint64_t *n_minimizers, uint64_t *clade_minimizers, double *distinct, double *clade_distinct);
/* the 4096 registers of one taxon (clade != 0: of its clade), for callers that reduce across devices themselves */
sh_status sh_k2_mindata_registers(sh_k2_mindata *md, uint32_t taxon, uint8_t *out /* 4096 */, int32_t clade);
/* host only, no GPU: Ertl's improved raw estimator over 4096 registers (values 0..53); element-wise maximum of n registers */
sh_status sh_k2_hll_estimate(const uint8_t *regs /* 4096 */, double *out);
sh_status sh_k2_mindata_merge_host(uint8_t *dst_regs, const uint8_t *src_regs, uint64_t n);
/* host only: the Kraken-style report with two columns after "direct reads": the clade's minimizer count and its distinct
 * estimate (8 tab-separated columns; rows, order, percent, rank codes and indentation as sh_k2_write_report; the unclassified
 * row, total_units - clade_reads[1] units, carries 0 for both).  Arrays are per internal taxon. */
sh_status sh_k2_write_minimizer_report(const sh_k2_taxnode *nodes, uint64_t n_nodes, const char *names, uint64_t names_len, const char *ranks,
                                       uint64_t ranks_len, const uint64_t *clade_reads, const uint64_t *direct_reads, const uint64_t *clade_minimizers,
                                       const uint64_t *clade_distinct, uint64_t total_units, const char *path);
/* the same from a database, per-unit calls and an accumulator (estimates rounded to the nearest integer) */
sh_status sh_k2_mindata_write_report(const sh_k2_db *db, const sh_k2_result *results, uint64_t n_units, sh_k2_mindata *md, const char *path);

/* `scrubby reads -c kraken2 -I DB -T .. -D ..`: Cleaner::run_kraken (cleaner.rs:288-330) in process: classify on the GPU,
 * write kraken.reads / kraken.report into workdir, then the taxid depletion of parse_classifier_output + clean_reads. */
typedef struct sh_kraken_config {
    const char *input[2];
    const char *output[2];
    uint32_t    n_files;            /* 2 = paired-end (kraken2 --paired) */
    int32_t     extract;
    const char *db;                 /* -I: database directory */
    const char *workdir;            /* -w, nullable: system temp dir */
    const char *const *taxa;        uint32_t n_taxa;
    const char *const *taxa_direct; uint32_t n_taxa_direct;
    double      confidence;         /* from -C "--confidence x"; < 0: default */
    int32_t     min_hit_groups;     /* <= 0: default */
    const char *json, *read_ids, *command;
    int32_t     device, threads;
    const char *classifier_args;    /* -C verbatim, nullable: echoed as settings.classifier_args in the JSON (report.rs:81) */
    int32_t     min_base_quality;   /* from -C "--minimum-base-quality n"; <= 0: no masking (FASTQ records only) */
    int32_t     quick;              /* from -C "--quick" */
    int32_t     report_minimizer_data;      /* from -C "--report-minimizer-data": also writes kraken.minimizer.report (8 columns) into
                                               the workdir; kraken.report keeps its 6 columns (the depletion reads it by position) */
} sh_kraken_config;
sh_status sh_kraken_run(const sh_kraken_config *cfg, sh_reads_result *out);

/* ---- Kraken arm: database build (DESIGN.md §7 "Database build").  Kraken 2's build rules as recalled from build_db.cc,
 * taxonomy.cc, estimate_capacity.cc and kraken2-build: PARITY UNPINNED, like the rest of the arm. ------------------------------ */
/* Host only (no GPU): an NCBI taxonomy reduced to the taxa a library uses, in taxo.k2d's layout. */
typedef struct sh_k2_taxonomy sh_k2_taxonomy;
typedef struct sh_k2_taxonomy_info {
    uint64_t n_nodes, names_len, ranks_len;
    int32_t  value_bits;            /* smallest b with 2^b >= n_nodes (>= 1), or the larger value the caller asked for */
    int32_t  pad;
    uint64_t n_map_entries;         /* sequence ids of the id map whose taxon is in nodes.dmp */
    uint64_t n_missing_taxa;        /* distinct taxids of the map (and of extra_taxids) that nodes.dmp lacks */
} sh_k2_taxonomy_info;
/* nodes.dmp + names.dmp (scientific names only) + seqid2taxid.map (nullable) + further taxids in use (nullable: those of
 * `kraken:taxid|n` headers).  Every used taxon and its ancestors up to the root (taxid 1) are kept, the rest dropped; internal
 * ids are breadth-first (0 the empty node, 1 the root), siblings in ascending external taxid.  A taxid that nodes.dmp lacks is
 * named once on stderr and its sequences are skipped. */
sh_status sh_k2_taxonomy_from_ncbi(const char *nodes_dmp, const char *names_dmp, const char *seqid2taxid_map,
                                   const uint64_t *extra_taxids, uint64_t n_extra, int32_t value_bits, sh_k2_taxonomy **out);
/* the host-depletion case: root -> one taxon (name NULL: "taxid <n>", rank NULL: "species"); every header maps to it */
sh_status sh_k2_taxonomy_single(uint64_t taxid, const char *name, const char *rank, int32_t value_bits, sh_k2_taxonomy **out);
sh_status sh_k2_taxonomy_info_get(const sh_k2_taxonomy *t, sh_k2_taxonomy_info *out);
/* nodes[n_nodes], names[names_len], ranks[ranks_len]; any of them may be NULL */
sh_status sh_k2_taxonomy_copy(const sh_k2_taxonomy *t, sh_k2_taxnode *nodes, char *names, char *ranks);
/* external -> internal id; 0 = not in the reduced taxonomy */
sh_status sh_k2_taxonomy_internal(const sh_k2_taxonomy *t, uint64_t external_id, uint32_t *internal_id);
/* FASTA header (without '>') -> internal taxon of its record: the id is the first whitespace-delimited token; a token holding
 * `kraken:taxid|<n>` takes <n>; ids joined by \x01 give the LCA of their taxa; 0 = no taxon, the record is skipped */
sh_status sh_k2_taxonomy_header_taxon(const sh_k2_taxonomy *t, const char *header, uint64_t len, uint32_t *internal_id);
sh_status sh_k2_taxonomy_free(sh_k2_taxonomy *t);

/* capacity = ceil(256 * n_sampled / load_factor) (load_factor <= 0: 0.7); then kraken2-build --max-db-size B (0: none): when
 * 4 * capacity > B, capacity = B / 4 and min_acceptable_hash = (uint64)((1 - B / (4 * needed)) * 2^64).  Host only. */
sh_status sh_k2_capacity_plan(uint64_t n_sampled, double load_factor, uint64_t max_db_size, uint64_t *estimate, uint64_t *capacity,
                              uint64_t *min_acceptable_hash);
/* the --max-db-size rule alone, on a capacity that is already known */
sh_status sh_k2_max_db_size(uint64_t needed_capacity, uint64_t max_db_size, uint64_t *capacity, uint64_t *min_acceptable_hash);
/* the database's down-sampling threshold (set before the first insert; written to opts.k2d, honoured by the classifier) */
sh_status sh_k2_set_min_acceptable_hash(sh_k2_db *db, uint64_t min_acceptable_hash);

typedef struct sh_k2_build_stats {
    uint64_t n_records;
    uint64_t n_segments;            /* (record, segment) work items of the launch */
    uint64_t n_runs;                /* minimizer runs handed to the table (a run that spans a segment border counts in both) */
    uint64_t size;                  /* distinct keys in the table after the call */
    float    ms;
} sh_k2_build_stats;
/* One launch over a batch of records in HBM: record r = d_bases[d_offsets[r], d_offsets[r + 1]) under internal taxon d_taxa[r]
 * (0, or one outside the taxonomy = skip; so is a record shorter than k).  d_bases must be readable up to the 8-byte boundary behind its last base.  One synchronisation per call.
 * SH_ERR_OOM when the table is full. */
sh_status sh_k2_insert_library_device(sh_k2_db *db, const uint8_t *d_bases, const uint64_t *d_offsets, const uint32_t *d_taxa,
                                      uint64_t n_records, void *stream, sh_k2_build_stats *stats);
/* Kraken 2's capacity estimator: the distinct minimizers m with (fmix64(m) & 1023) < 4, accumulated over every batch given to
 * one estimator; *n_sampled = their number so far (estimate = 256 * n_sampled: sh_k2_capacity_plan). */
typedef struct sh_k2_estimator sh_k2_estimator;
sh_status sh_k2_estimator_create(const sh_k2_opts *opts, int device, sh_k2_estimator **out);
sh_status sh_k2_estimate_capacity_device(sh_k2_estimator *est, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_records,
                                         void *stream, uint64_t *n_sampled);
sh_status sh_k2_estimator_free(sh_k2_estimator *est);

/* `scrubby-hip k2-build`: library FASTA files (plain, gzip, bzip2, xz) + taxonomy -> hash.k2d / opts.k2d / taxo.k2d */
typedef struct sh_k2_build_config {
    const char *const *input;  uint32_t n_input;
    const char *taxonomy_dir;       /* holds nodes.dmp and names.dmp; NULL: single-taxon mode */
    const char *seqid2taxid;        /* nullable (headers may carry kraken:taxid|n) */
    uint64_t    taxid;              /* single-taxon mode: every record's taxon */
    const char *name, *rank;        /* single-taxon mode, nullable */
    const char *output_dir;
    int32_t     k, l, minimizer_spaces;     /* 0: 35, 31, 7; minimizer_spaces < 0: no spaced seed */
    int32_t     value_bits;         /* 0: the minimum for the taxonomy */
    uint64_t    capacity;           /* 0: estimate it (a pass of its own over the input) */
    double      load_factor;        /* <= 0: 0.7 */
    uint64_t    max_db_size;        /* bytes, 0: unlimited */
    uint64_t    chunk_bytes;        /* bases per batch, 0: 256 MiB; a longer record is cut (k - 1 bases repeated) */
    int32_t     device, pad;
    int32_t     mask_low_complexity;        /* 1: both passes mask every batch on the GPU first (sh_k2_mask_device, masked bases
                                             * become 'x'); 0: the library is taken as given */
    int32_t     mask_window, mask_threshold;        /* 0: 64, 20 */
    int32_t     protein;            /* 1: kraken2-build --protein: the library is amino-acid FASTA, the defaults k 15, l 12, no minimizer
                                     * spaces (minimizer_spaces 0 or negative); mask_low_complexity is then SH_ERR_BAD_ARG */
} sh_k2_build_config;
typedef struct sh_k2_build_result {
    uint64_t n_records, n_skipped, n_bases, n_batches, n_cuts;
    uint64_t n_runs, size, capacity, n_nodes, n_sampled, estimate, min_acceptable_hash;
    int32_t  value_bits, pad;
    double   s_taxonomy, s_estimate, s_fill, s_save, s_read, s_total;   /* s_read: reading + parsing + upload inside the two passes */
    uint64_t n_masked_bases;        /* bases of the library the fill pass masked (each once, whatever the cuts) */
    double   s_mask;                /* the mask calls of both passes (inside s_estimate and s_fill) */
} sh_k2_build_result;
sh_status sh_k2_build_run(const sh_k2_build_config *cfg, sh_k2_build_result *out);

/* ---- low-complexity masking before the build (DESIGN.md §7 "Low-complexity masking"): kraken2-build's k2mask / dustmasker step.
 * Symmetric DUST as recalled (Morgulis et al. 2006), in integers: PARITY WITH k2mask UNPINNED, like the rest of the section.
 * Inside a maximal run of ACGTacgt (any other byte and a record border end it), an interval of triplets [i, j], i < j, of at most
 * window - 2 triplets has the score r / l, r = sum over triplet codes of c (c - 1) / 2, l = j - i; it is perfect when
 * 10 r > threshold * l and no interval inside it scores strictly higher; the bases of every perfect interval are masked. */
typedef struct sh_k2_mask_stats {
    uint64_t n_bases, n_masked;
    uint64_t n_items;               /* (record, tile) work items of the launch */
    float    ms;
    int32_t  pad;
} sh_k2_mask_stats;
/* Masks a batch in HBM in place: record r = d_bases[d_offsets[r], d_offsets[r + 1]).  window 0 = 64 (allowed: 8 .. 64),
 * threshold 0 = 20 (>= 1).  replacement = the byte masked bases become ('x' is what kraken2-build uses: not a nucleotide, so the
 * minimizer scan restarts behind it), or 0 = soft masking (lower case).  d_bases must be readable up to the 8-byte boundary
 * behind its last base, as for sh_k2_insert_library_device.  One synchronisation per call. */
sh_status sh_k2_mask_device(uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_records, int32_t window, int32_t threshold,
                            int32_t replacement, void *stream, sh_k2_mask_stats *stats);
/* The same result on the CPU (no GPU), written as the streaming sdust programme is: the mirror the tests call; the GPU paths
 * never do.  stats may be NULL (ms = 0, n_items = 0). */
sh_status sh_k2_mask_host(uint8_t *bases, const uint64_t *offsets, uint64_t n_records, int32_t window, int32_t threshold,
                          int32_t replacement, sh_k2_mask_stats *stats);
/* `scrubby-hip k2-mask`: FASTA in (plain, gzip, bzip2, xz), masked FASTA out (container by extension), headers untouched */
typedef struct sh_k2_mask_config {
    const char *input, *output;
    int32_t     window, threshold;  /* 0: 64, 20 */
    int32_t     replacement;        /* 0: 'x' */
    int32_t     soft;               /* 1: lower case instead of the replacement byte */
    int32_t     line_width;         /* bases per output line (the CLI's default is 60); 0: a record's sequence on one line */
    int32_t     device;
    uint64_t    chunk_bytes;        /* bases per batch, 0: 256 MiB; the output does not depend on it */
} sh_k2_mask_config;
typedef struct sh_k2_mask_result {
    uint64_t n_records, n_bases, n_masked_bases, n_batches, n_cuts;
    double   s_mask, s_total;
} sh_k2_mask_result;
sh_status sh_k2_mask_run(const sh_k2_mask_config *cfg, sh_k2_mask_result *out);

/* ---- multi-GPU: the one exchange of the read-sharded path (HashSet union of cleaner.rs:564-570) --------------
 * d_flags[n] (1 = host) -> d_bits[(n + 7) / 8], bit i of byte j = record 8j + i; each rank packs its own slice and the disjoint
 * slices are all-gathered over RCCL (scrubby_amd/dist.py). */
sh_status sh_pack_flags_device(const uint8_t *d_flags, uint64_t n, uint8_t *d_bits, void *stream);

/* ---- micro-benchmarks for the roofline (bench.py) ---------------------------------------- */
/* random 16-B slot gathers over the index table; returns achieved GB/s of useful bytes */
sh_status sh_bench_gather(const sh_index *idx, uint64_t n_probes, int32_t iters, double *out_gbs_useful, double *out_ms);
/* Test aid: the krmq tree of the long join (csrc/sh_rmq_tree.h) on the device - one lane runs a random insert / erase / query sequence with
 * heavily tied priorities (the generator of oracle/mm_rmq.c's mmo_rmq_trace) and returns, per query, the element the tree answered with
 * (its i, or -1).  lds = 0: nodes in a pool in HBM (RqPool); lds = 1: the whole tree in LDS (RqLds, 4096 nodes: *n_out = -100 when the sequence
 * holds more at once), one lane; lds = 2: that tree with the insertions and erasures done by the whole wave (rq_insert_w / rq_erase_w).  out: host array of n_ops int64; *n_out < 0: a guard of the tree code tripped. */
sh_status sh_dbg_rmq_trace(int32_t device, uint64_t seed, int32_t n_ops, int32_t key_range, int32_t fifo, int32_t lds, int64_t *out, int64_t *n_out);
/* test aid: the wave primitives of csrc/sh_wave.h (DPP scans / reductions / broadcasts) on one wave of inputs: 12 x 64 int32 and 9 x 64 uint64
 * results in the order of k_dbg_wave_ops (tests/test_wave_ops_gpu.py compares them with numpy) */
sh_status sh_dbg_wave_ops(int32_t device, const int32_t *in32, const uint64_t *in64, int32_t bcast_lane, int32_t *out32, uint64_t *out64);
/* Test aids: the two alignment kernels of the extension stage called directly (csrc/sh_dbg_align.hip; tests/test_ksw_gpu.py compares them
 * with the oracle's mma_ksw_extd2 / mma_ksw_ll bit for bit).  A batch of cases runs in one launch, one 64-lane block per case.  The sequences are
 * codes 0..4 at byte offsets of one host blob, so a case can start at any alignment.
 * route 0: the case goes through ksw_extd2_wave as the short-read stage calls it (state and directions in LDS / directions in HBM / both in
 * HBM); route 1: through lr_align_pair as the long-read stage calls it (never all in LDS).  Every wave's scratch is sized for the largest
 * case of the batch that is not marked `unsized`; an unsized case must be one the code under test then turns away (else SH_ERR_BAD_ARG).
 * Result: the eleven fields of ksw_extz_t, the storage form taken (0 / 1 / 2; route 1 turned away by lr_align_pair: -1 = direction bytes
 * beyond the scratch, -2 = bases beyond it, fields as after a reset) and where the case's CIGAR words (len << 4 | op) start in out_cigar, which holds
 * cigar_cap >= the sum of qlen + tlen over the batch words. */
typedef struct sh_dbg_ksw_case {
    uint64_t q_off, t_off;
    int32_t qlen, tlen, a, b, sc_ambi, q, e, q2, e2, w, zdrop, end_bonus, flag, route, unsized, pad;
} sh_dbg_ksw_case;
typedef struct sh_dbg_ksw_result {
    int32_t max, zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, reach_end, n_cigar, form;
    uint64_t cigar_off;
} sh_dbg_ksw_result;
sh_status sh_dbg_ksw_extd2(int32_t device, const uint8_t *blob, uint64_t blob_len, const sh_dbg_ksw_case *cases, int32_t n_cases,
                           sh_dbg_ksw_result *out, uint32_t *out_cigar, uint64_t cigar_cap);
/* the local alignment behind the inversion test (lr_ksw_ll_wave), rows sized as the long-read working memory sizes them: the score and the
 * end of the alignment in the query (qe) and the target (te) */
typedef struct sh_dbg_ll_case { uint64_t q_off, t_off; int32_t qlen, tlen, a, b, sc_ambi, gapo, gape, pad; } sh_dbg_ll_case;
typedef struct sh_dbg_ll_result { int32_t score, qe, te, pad; } sh_dbg_ll_result;
sh_status sh_dbg_ksw_ll(int32_t device, const uint8_t *blob, uint64_t blob_len, const sh_dbg_ll_case *cases, int32_t n_cases, sh_dbg_ll_result *out);
/* Test aids: the region bookkeeping between "a read's chains" and "a region survives mm_filter_regs" - mm_gen_regs' order, mm_set_parent,
 * mm_select_sub, the split / insert steps of mm_align_skeleton - called directly (csrc/sh_dbg_align.hip; tests/test_regs_gpu.py compares with the
 * oracle's mma_align_read_rows / mma_chain_post and with the plain model tests/regs_ref.py, integers only).
 *
 * sh_dbg_regs_short: align_read_wave of csrc/sh_align.h, one wave per read, over caller-made chains.  ref_packed / cstart: the reference as 4-bit
 * codes and the contig starts (n_contigs + 1); bases / offsets: the reads (ASCII); cx / cq: the anchors (x = strand << 63 | contig << 32 | last
 * reference base, q = last query base); recs / head: the chain records with their `next` links exactly as given, head[read] = the first record
 * of the read or ~0u.  mode[read]: 0 every region, 1 flag_only (stops at the first survivor), 2 top_z: the record with the read's largest z
 * alone, through the AlignLdsTop instance (modes 0 and 1: AlignLds).  Every wave's scratch is laid out for (max_read_len, reg_cap) as the
 * product lays it out and lies between two guard bands of 4 KiB of a known byte; out.guard = how many of their bytes changed.
 * out.done = 0: the read was given up with out.overflow (2 more chains than reg_cap, 3 more primaries than room, 4 query beyond the scratch,
 * 5 reference window beyond it, 6 a split needs a slot beyond the region arrays).  book: row_cap pairs per read - the record index of each region
 * mm_select_sub kept, in order, and of the record of its parent; keep: row_cap rows of eight per read - rs, re, qs, qe, mlen, blen, dp_max, cnt of
 * each surviving region; out.n_book / out.n_keep count every row, stored or not.
 * Refused with SH_ERR_BAD_ARG before any launch - these are what the chaining kernels guarantee the product: a `next` chain that does not end in
 * ~0u within n_recs steps or leaves the table; a record with no anchors, anchors outside cx / cq, a negative score, or a z that is not chain_z of
 * its first anchor; anchors of a record not strictly ascending in x and in q, not on one contig and strand, or whose k bases do not lie inside
 * the contig and inside the read; an empty read; k < 1, e < 1, reg_cap < 1, max_read_len < 1; a mode other than 0, 1, 2. */
typedef struct sh_dbg_chain_rec { uint32_t next, cnt; int32_t score; uint32_t key_f, key_i, yfl; uint64_t off, z; } sh_dbg_chain_rec;
typedef struct sh_dbg_align_params {
    int32_t k, min_cnt, min_sc, max_gap, bw, bw_long;
    int32_t a, b, q, e, q2, e2, sc_ambi, zdrop, zdrop_inv, end_bonus, min_dp_max, best_n;
    float pri_ratio, mask_level, max_clip_ratio;
    int32_t lemma, unc_max;
} sh_dbg_align_params;
typedef struct sh_dbg_regs_out { int32_t n_aligned, n_regs, dp_max; uint32_t sig, overflow; int32_t done; uint32_t n_book, n_keep, guard, pad; } sh_dbg_regs_out;
sh_status sh_dbg_regs_short(int32_t device, const uint8_t *ref_packed, const uint64_t *cstart, uint32_t n_contigs, const uint8_t *bases,
                            const uint64_t *offsets, uint32_t n_reads, const uint64_t *cx, const uint32_t *cq, uint64_t n_anchors,
                            const sh_dbg_chain_rec *recs, uint32_t n_recs, const uint32_t *head, const sh_dbg_align_params *params,
                            uint32_t reg_cap, uint32_t max_read_len, const int32_t *mode, uint32_t row_cap,
                            sh_dbg_regs_out *out, uint32_t *book, int32_t *keep);
/* sh_dbg_regs_long: lr_set_parent0, then lr_select_sub0 (with lr_sync_regs0) of csrc/sh_long.h, one lane per case, over caller-made regions.
 * tab: n_rows rows of nine ints - score, cnt, qs, qe, rs, re, rev, rid, inv; case i is the n rows from off.  rows: per kept region of case i, from
 * row off on, six ints: its row in the case's table, id, parent, subsc, n_sub, strand_retained; n_kept[i] = how many.
 * Refused before any launch: a case outside tab, n < 1 or n > 4096 (the scratch of a case), a region with qe <= qs. */
typedef struct sh_dbg_lreg_case { uint64_t off; int32_t n, min_diff, best_n, min_strand_sc; float mask_level, pri_ratio; } sh_dbg_lreg_case;
sh_status sh_dbg_regs_long(int32_t device, const int32_t *tab, uint64_t n_rows, const sh_dbg_lreg_case *cases, int32_t n_cases, int32_t *n_kept, int32_t *rows);
/* Test aid: the variants of the chaining DP (mg_lchain_dp) and of the backtrack (mg_chain_backtrack) in csrc/sh_chain.h, called directly
 * (csrc/sh_dbg_chain.hip; tests/test_chain_gpu.py compares them with the oracle's mmo_chain_arrays, integers only).  One launch per DP variant,
 * one block per case, with the block size the product runs the variant with.
 * x / q: n_total sorted anchors (x = strand<<63 | contig<<32 | ref pos, q = query pos; bit 31 of q marks the first anchor of a cluster where
 * the variant expects it: 6, 7 and the backtrack 5); a case reads n of them from `off` (variant 3: in any order, it sorts them itself).
 * dp: 0 = none, f / p are taken from f_in / p_in; 1 chain_dp (LargeStore); 2 chain_dp_mask (SliceStore); 3 chain_dp_mask over SmallStore<32>,
 *     filled with set_raw + sort_finalize; 4 chain_dp_wave; 5 chain_dp_ring; 6 par_fill_block (256 threads); 7 par_fill_tiled (512 threads, g_min).
 * bt: 0 = none; 1 backtrack_small; 2 backtrack_mask; 3 backtrack_heap; 4 backtrack_wave_top; 5 backtrack_block_top (a zeroed ChainSink, at most
 *     top_cap candidates); 6 first_chain_quick.  bt 1..4 and 6 go with dp 0..5 (after dp 3 over the SmallStore: bt 2 only), bt 5 with dp 0, 6, 7 (dp 0 and 6: 256 threads).
 * The outputs of case i start at o_i = the sum of n over the cases before it, in f_in, p_in, f, p, t (what the store holds at the end) and,
 * times five, in chains: (zi, end_i, score, cnt, zf) per accepted chain in visit order, recorded by the test emitter (whose done() is false).
 * ret: the DP's return value; bt_ret: backtrack 5's return value, 6's result.  A case its variant cannot take (n > 64 for the masks; n > 32,
 * q > 65535 or k * n > 65535 for the SmallStore; max_iter > 8000 for the ring; unsorted anchors; a combination not listed) is SH_ERR_BAD_ARG
 * before any launch. */
typedef struct sh_dbg_chain_case {
    uint64_t off;
    int32_t n, qlen, dp, bt, g_min, first_only, top_cap, pad;
    int32_t k, is_sr, min_cnt, min_sc, max_gap, max_gap_ref, max_frag_len, bw, max_skip, max_iter;
    float chain_gap_scale, chain_skip_scale;
} sh_dbg_chain_case;
typedef struct sh_dbg_chain_result { int32_t ret, bt_ret, n_u, best, n_emit, pad; } sh_dbg_chain_result;
sh_status sh_dbg_chain(int32_t device, const uint64_t *x, const uint32_t *q, uint64_t n_total, const sh_dbg_chain_case *cases, int32_t n_cases,
                       const int32_t *f_in, const int32_t *p_in, sh_dbg_chain_result *out, int32_t *f, int32_t *p, int32_t *t, int32_t *chains);
/* Test aid: the stable block sort of the repeat path (block_merge_sort in csrc/sh_wave.h: the LDS sort classes, the giant reads' tiles and the
 * group probe share it), called directly (csrc/sh_dbg_chain.hip; tests/test_block_sort_gpu.py compares with numpy's stable argsort).  One block
 * of nthr threads (64, 128, 256 or 512) per case sorts the n pairs (x[off + i], q[off + i]), 1 <= n <= 4096, by x in LDS, equal x in input
 * order, and stores them at the same place in out_x / out_q; one launch per thread count.  Pairs no case covers come back as (0, ~0u).  Another
 * n or thread count, or a case outside the arrays: SH_ERR_BAD_ARG before any launch. */
typedef struct sh_dbg_sort_case { uint64_t off; int32_t n, nthr; } sh_dbg_sort_case;
sh_status sh_dbg_block_sort(int32_t device, const uint64_t *x, const uint32_t *q, uint64_t n_total, const sh_dbg_sort_case *cases, int32_t n_cases,
                            uint64_t *out_x, uint32_t *out_q);
/* Test aid: stage_anchors of csrc/sh_chain.h - the anchors of a short read built in the LDS sort buffer of the kernel that sorts them - called
 * directly (csrc/sh_dbg_chain.hip; tests/test_stage_anchors_gpu.py).  records: 16-byte seed records as four u32 (.x,.y = position word or
 * slot << 28 | n, .z = occurrences, .w = qpos << 1 | strand); positions: the occurrence lists.  Case i is a read of n_seed (1..64) records from
 * rec_off with qlen bases and the range [c0, c0 + m), 1 <= m <= 4096, of its anchors in generation order, staged by one block of nthr threads
 * (64, 128, 256 or 512) into out_x / out_q [out_off, out_off + m); ref_x / ref_q get the same range from a plain loop of one thread over the
 * seeds seed_filter keeps (make_anchor per occurrence), total[i] the read's anchor count.  The filter is the occurrence cut at max_occ with
 * mm_seed_select's streaks (occ_dist, max_max_occ; occ_dist = 0: the plain cut).  A range that reaches past total[i] is not staged; pairs no
 * case covers come back as (0, ~0u).  A case or an occurrence list outside its array: SH_ERR_BAD_ARG before any launch. */
typedef struct sh_dbg_stage_case { uint64_t rec_off, out_off; int32_t n_seed, qlen, nthr, pad; uint32_t c0, m; } sh_dbg_stage_case;
sh_status sh_dbg_stage_anchors(int32_t device, const uint32_t *records, uint64_t n_records, const uint64_t *positions, uint64_t n_positions,
                               int32_t k, int32_t max_occ, int32_t max_max_occ, int32_t occ_dist, const sh_dbg_stage_case *cases, int32_t n_cases,
                               uint64_t n_out, uint64_t *out_x, uint32_t *out_q, uint64_t *ref_x, uint32_t *ref_q, uint32_t *total);
/* Test aid: the long join of csrc/sh_long.h - mg_lchain_rmq's scoring pass in every form the product runs, and the two backtracks behind it -
 * called directly (csrc/sh_dbg_long.hip; tests/test_long_join_gpu.py compares with the oracle's mmo_lchain_rmq_fill / mmo_backtrack_arrays and
 * the plain model of tests/long_join_ref.py, integers only).  One launch per instance (they differ in LDS), one 64-lane block per case.
 * x / y: n_total anchors, y = q_span << 32 | qpos; a case reads n of them from `off`, ascending in x.
 * fill: 0 = none, f / p are taken from f_in / p_in; 1..5 lr_rmq_fill<512,F,F>, <4096,F,F>, <4096,F,FAT>, <1024,TREE,F>, <4096,TREE,F> as
 *     lr_chains_wave calls them (the TREE ones with an LDS tree of 1664 / 1792 nodes); 6 lr_rmq_fill_tree (t zeroed, pools of n + 2 nodes);
 *     7 the case cut at cuts[cut_off .. cut_off + n_cut) (indices into the case, each a stretch start), every run filled by
 *     lr_rmq_fill<ring,TREE,F> with p_base = the run's start and bmin at start / 64 + run, as lr_coop_take calls it; 8 lr_coop_fill<ring>
 *     itself when n >= coop_min (else as 4 / 5): the cases of one (ring, q_cap) that agree on every option the fill reads (k, max_gap,
 *     bw_long, max_skip, rmq_inner_dist, rmq_size_cap, pen_gap, pen_skip) share one launch and one queue of q_cap slots, one owner block each
 *     (q_cap 0: every run stays with its owner) - a run is filled with the options of the wave that takes it, and in the product a launch has
 *     one set of them.  ring: 1024 or 4096, read by 7 and 8.
 * bt: 0 = none; 1 lr_backtrack0; 2 lr_backtrack_wave - over the candidates f >= min_sc compacted and sorted by lr_sort, t zeroed, as
 *     lr_chains_wave sets it up; max_drop is what the product passes bw_long for.  Skipped when the fill returned false.
 * The outputs of case i start at o_i = the sum of n over the cases before it in f_in, p_in, f, p, t, v and u (at most min(cap_u, n) chains).
 * On the device every array a case's block writes (f, p, t, v, u, pri, bmin of n / 64 + 1 entries plus one per run, the sort keys, the node
 * pools) lies between two 4 KiB bands of one byte value; guard = the number of band bytes that changed.
 * SH_ERR_BAD_ARG before any launch: a case outside the arrays, n < 1, x not ascending, a q_span other than k (the ring scores with k), the low
 * words of x and y negative or their sum beyond int32 (the priority adds them as int32), a cut that is no stretch start (x jumps by more than
 * max(max_gap, bw_long) or the high word changes), uploaded f / p that are no chaining state, a variant not listed. */
typedef struct sh_dbg_long_case {
    uint64_t off, cut_off;
    int32_t n, fill, bt, ring;
    int32_t k, max_gap, bw_long, max_skip, rmq_inner_dist, rmq_size_cap, min_cnt, min_sc, coop_min, coop_run, max_drop, cap_u, n_cut, q_cap;
    float pen_gap, pen_skip;
} sh_dbg_long_case;
typedef struct sh_dbg_long_result { int32_t ok, n_tie, n_u, n_v, best, ovf, n_z, pad; uint64_t guard; } sh_dbg_long_result;
sh_status sh_dbg_long_join(int32_t device, const uint64_t *x, const uint64_t *y, uint64_t n_total, const sh_dbg_long_case *cases, int32_t n_cases,
                           const int32_t *f_in, const int32_t *p_in, const int32_t *cuts, sh_dbg_long_result *out,
                           int32_t *f, int32_t *p, int32_t *t, uint64_t *u, int32_t *v);
/* lr_sort of csrc/sh_long.h alone: one wave per case sorts the n >= 0 distinct pairs (k[off + j], v[off + j]) ascending; out_i = each pair's
 * place j in the input.  The arrays reach as far as the cases say; what no case covers comes back unchanged with out_i = ~0u. */
typedef struct sh_dbg_lr_sort_case { uint64_t off; int32_t n, pad; } sh_dbg_lr_sort_case;
sh_status sh_dbg_lr_sort(int32_t device, const uint64_t *k, const uint64_t *v, const sh_dbg_lr_sort_case *cases, int32_t n_cases,
                         uint64_t *out_k, uint64_t *out_v, uint32_t *out_i);

/* Test aid: the three minimizer state machines of csrc/sh_sketch.h, called directly (csrc/sh_dbg_sketch.hip; tests/test_sketch_gpu.py compares
 * them with the oracle's mmo_sketch, integers only).  One lane per sequence, one launch per call.  bases / offsets: host arrays, sequence i is
 * bases[offsets[i] .. offsets[i + 1]) in ASCII (decoded with sh_nt4).  form 0: SketchState<w> over the whole sequence; 1: SketchPacked<w>, driven
 * in blocks of w steps with block_end() after each, every push through sh_packed_entry, one push for minimum and tie entries as the read kernel
 * has it; 2: SketchStateDyn with its ring in HBM.  The pushes of sequence i come back in emission order as (hash, y = pos << 1 | strand) at
 * hash / y [offsets[i] - offsets[0] + i ..], room for len + 1 of them; count[i] = how many there were (a push beyond the room is counted, not
 * written).  hash and y hold offsets[n_seq] - offsets[0] + n_seq entries.  w outside {5, 10, 11, 19}, even k, k > 23 (form 1) or 27, a sequence
 * of more than 1024 bases (form 1): SH_ERR_BAD_ARG before any launch. */
sh_status sh_dbg_sketch(int32_t device, const uint8_t *bases, const uint64_t *offsets, int32_t n_seq, int32_t w, int32_t k, int32_t form,
                        uint64_t *hash, uint32_t *y, int32_t *count);
/* Test aid: the front end of sh_classify_device alone (the read kernel k_sketch_probe, or the segment-parallel long-read kernels, as the
 * context chooses), on a chunk in HBM of at most the context's max_reads reads of at most its max_read_len bases.  Resets the counters,
 * launches, synchronises and copies out to host arrays, per read r:
 *   k1info[r]   as the kernels leave it (read kernel: minimizers | seeds << 16 | tandem << 31; long: minimizers after thinning | seeds << 16);
 *   route[r]    the work list that names the read: 0 none (decided with no seed), 1 work_small, 2 work_big, 4 work_resketch; more than one bit or
 *               bit 7 (named twice by one list) is a fault of the front end;
 *   records     its seed records, four words each (x, y = the slot's payload, z = occurrences | SH_REC_PREV_SAME, w = qpos << 1 | strand), at
 *               records[4 * rec_off[r] .. 4 * rec_off[r + 1]): the read kernel's first min(seeds, seed_cap), the long front end's all;
 *   mz_hash / mz_y [mz_off[r] .. mz_off[r + 1])   long front end only: its minimizers as they stand after mm_seed_mz_flt's thinning.
 * rec_off and mz_off hold n_reads + 1 entries; rec_cap / mz_cap: room in records (records of four words) and mz_hash / mz_y (n_bases + 1 always
 * suffices; less than needed is SH_ERR_BAD_ARG).  info[5]: front end (1 read kernel, 2 long, 0 neither), seed_cap, and the lengths of work_small,
 * work_big and work_resketch. */
sh_status sh_dbg_front_end(sh_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases,
                           uint32_t *k1info, uint8_t *route, uint64_t *rec_off, uint32_t *records, uint64_t rec_cap,
                           uint64_t *mz_off, uint64_t *mz_hash, uint32_t *mz_y, uint64_t mz_cap, int32_t *info);
/* Test aid: the flag-only shortcuts over the repeat path's list alone (tests/test_local_cluster_gpu.py), on a short-read context with
 * SH_F_CIGAR (anything else, a non-null d_trace, or options that leave ChainParams::ext_lemma at 0 without SCRUBBY_HIP_NO_LEMMA: SH_ERR_BAD_ARG).
 * Resets the counters and a flags buffer of its own, runs the front end, then under mask (bit 0: k_pair_pass over the list, bit 1:
 * k_local_cluster, always its counting instance) what sh_classify_device runs there, and nothing behind it.  Copies out, per read r:
 *   k1info[r]   as the read kernel left it;
 *   route[r]    bit 0: the front end put the read on the repeat list; bit 1: the list the shortcuts left over names it; bit 7: a list names it twice;
 *   flags[r]    1: a shortcut decided the read (mapped), else 0;
 * and for the call lc_why[11] (how each read of k_local_cluster's list ended: tried, no singleton, a seed above mid_occ, singletons apart,
 * window, K size, margin, lemma, decided, decided with seeds filtered, seed count not 2 .. 64), pair_mid[4] (the pair pass's middle checks)
 * and info[4]: the length of the repeat list, of the leftover list, whether k_pair_pass ran, whether k_local_cluster ran. */
sh_status sh_dbg_repeat_shortcuts(sh_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases,
                                  const void *d_trace, int32_t mask, uint32_t *k1info, uint8_t *route, uint8_t *flags,
                                  uint32_t *lc_why, uint32_t *pair_mid, int32_t *info);

/* ---- Kraken arm: database inspection (DESIGN.md §7 "Database inspection"): what kraken2-inspect prints, as recalled from
 * dump_table.cc and CompactHashTable::GetValueCounts: PARITY WITH kraken2-inspect UNPINNED, like the rest of the arm.  One pass over
 * the table in HBM: every non-empty cell (the whole cell is not 0) counts under its value, cell & ((1 << value_bits) - 1).  An
 * occupied cell whose value is 0 or >= n_nodes is a bad value: counted in n_bad_values and nowhere else. */
typedef struct sh_k2_inspect_stats { uint64_t n_cells, n_occupied, n_bad_values; float ms; int32_t pad; } sh_k2_inspect_stats;
/* counts of the table as it is now (after any inserts).  d_counts: n_nodes uint64 in HBM, overwritten.  Asynchronous on stream unless stats != NULL. */
sh_status sh_k2_value_counts_device(const sh_k2_db *db, uint64_t *d_counts, void *stream, sh_k2_inspect_stats *stats);
sh_status sh_k2_value_counts(const sh_k2_db *db, uint64_t *counts /* host, n_nodes */, sh_k2_inspect_stats *stats);
#define SH_K2_INSPECT_ZERO_COUNTS 1   /* kraken2-inspect --report-zero-counts: also the taxa whose clade count is 0 */
#define SH_K2_INSPECT_MPA         2   /* kraken2-inspect --use-mpa-style: "d__A|p__B<tab>clade" per taxon of a lettered rank */
/* host only, no GPU: the report over any taxonomy in taxo.k2d's layout.  flags: SH_K2_INSPECT_ZERO_COUNTS, SH_K2_INSPECT_MPA.  header (nullable) is written first, verbatim.  path NULL or "-" = stdout. */
sh_status sh_k2_counts_report(const sh_k2_taxnode *nodes, uint64_t n_nodes, const char *names, uint64_t names_len, const char *ranks, uint64_t ranks_len,
                              const uint64_t *counts, int32_t flags, const char *header, const char *path);
/* the seven '#' lines of a database into buf (the cap / len convention of the hit-list formatter above) */
sh_status sh_k2_inspect_header(const sh_k2_db *db, char *buf, uint64_t cap, uint64_t *len);
/* `scrubby-hip k2-inspect`: open, count, write the header and the report.  skip_counts: the header only, nothing is launched.
 * Bad values: SH_ERR_IO that names their number, no report.  A header size that differs from the occupied cells is named once on
 * stderr; the header's value is printed all the same. */
typedef struct sh_k2_inspect_config { const char *db, *output; int32_t skip_counts, report_zero_counts, use_mpa_style, device; } sh_k2_inspect_config;
typedef struct sh_k2_inspect_result { uint64_t capacity, size_header, n_occupied, n_bad_values, n_nodes, n_taxa_with_minimizers; double s_open, s_count, s_report, s_total; } sh_k2_inspect_result;
sh_status sh_k2_inspect_run(const sh_k2_inspect_config *cfg, sh_k2_inspect_result *out);

/* ---- Kraken arm: abundance re-estimation (DESIGN.md §7 "Abundance re-estimation"): bracken-build's k-mer distribution on the GPU
 * and Bracken's estimate on the host.  The method of Lu et al. 2017 as this project states it; Bracken's sources were not at hand:
 * PARITY WITH Bracken's OWN PROGRAMS UNPINNED, like the rest of the arm.
 * Codes: every k-mer of a library record has the code the hit lists give it (internal taxon of its minimizer, 0, or
 * SH_K2_HIT_AMBIGUOUS).  Windows: for a read length L (k <= L <= 1024) and W = L - k + 1, a record of len bases under internal taxon
 * g != 0 has len - L + 1 windows (none when len < L); window p holds k-mers p .. p + W - 1 and its call is Kraken 2's ResolveTree
 * over the counts of its codes other than 0 and ambiguous (total W, confidence 0, no minimum-hit-groups test; no counted code: call
 * 0).  Distribution: the map (g, call) -> windows, and per g the windows in all, unclassified ones included.  It does not depend on
 * batching, record order, or where a long record is cut (pieces repeat L - 1 bases, so every window lies in exactly one piece).
 * Several accumulators (one per GPU) add: entries add per (genome, mapped), totals add per genome. */
typedef struct sh_k2_distrib sh_k2_distrib;            /* accumulator of one database and one read length, in HBM */
typedef struct sh_k2_distrib_entry { uint32_t genome, mapped; uint64_t windows; } sh_k2_distrib_entry;      /* internal ids */
typedef struct sh_k2_distrib_stats {
    uint64_t n_records;
    uint64_t n_windows;             /* windows of the call */
    uint64_t n_items;               /* (record, stretch of window starts) work items */
    uint64_t n_big;                 /* stretches finished by the second instance (a window with more distinct taxa than the LDS table holds) */
    float    ms;
    int32_t  pad;
} sh_k2_distrib_stats;
/* window starts per work item of the window kernel */
uint32_t sh_k2_distrib_stretch(void);
/* the database must outlive the accumulator.  SH_ERR_OOM names the size */
sh_status sh_k2_distrib_create(const sh_k2_db *db, int32_t read_len, sh_k2_distrib **out);
sh_status sh_k2_distrib_reset(sh_k2_distrib *d);
sh_status sh_k2_distrib_free(sh_k2_distrib *d);
/* Adds the windows of a batch in HBM: layout, taxon rules (0 or >= n_nodes = skip) and the readable tail as for
 * sh_k2_insert_library_device.  Calls add up in any batching.  One synchronisation per call (a second one, and the batch again,
 * when the code scratch has to grow).  SH_ERR_OOM names the size when the (genome, mapped) table is full: the accumulator then
 * refuses further batches until it is reset. */
sh_status sh_k2_distrib_add_device(sh_k2_distrib *d, const uint8_t *d_bases, const uint64_t *d_offsets, const uint32_t *d_taxa, uint64_t n_records,
                                   void *stream, sh_k2_distrib_stats *stats);
/* the two kernels' shares of the last call's ms (measurement aid; any pointer may be NULL) */
sh_status sh_k2_distrib_last_ms(const sh_k2_distrib *d, float *ms_codes, float *ms_windows);
sh_status sh_k2_distrib_count(sh_k2_distrib *d, uint64_t *n_entries);
/* entries sorted by (genome, mapped), call 0 included; totals: n_nodes uint64 by internal id (any pointer may be NULL) */
sh_status sh_k2_distrib_copy(sh_k2_distrib *d, sh_k2_distrib_entry *entries, uint64_t *totals);
/* Host only (no GPU), over host arrays.
 * _write: Bracken's database<L>mers.kmer_distrib: the header line "mapped_taxid\tgenome_taxids:kmers_mapped:total_genome_kmers", then
 * one line per mapped taxon, external ids, ascending: "<mapped>\t<g>:<windows>:<total(g)>" with the entries separated by single
 * spaces and genomes ascending.  Rows for call 0 are not written (the totals still include those windows).  An id outside the
 * taxonomy is SH_ERR_BAD_ARG.
 * _read: that file back into entries sorted by (genome, mapped) and totals (n_nodes, zeroed first).  entries NULL or cap too small:
 * only *n_entries is set.  A taxid outside the taxonomy is named once on stderr and skipped; a malformed line is SH_ERR_IO naming
 * the line. */
sh_status sh_k2_distrib_write(const sh_k2_distrib_entry *entries, uint64_t n, const uint64_t *totals, const uint32_t *external, uint64_t n_nodes,
                              int32_t read_len, const char *path);
sh_status sh_k2_distrib_read(const char *path, const uint32_t *external, uint64_t n_nodes, sh_k2_distrib_entry *entries, uint64_t cap,
                             uint64_t *n_entries, uint64_t *totals);
/* Bracken's estimate.  level: one of D K P C O F G S (the rank names of sh_k2_write_report).  lvl(x) = the nearest ancestor-or-self
 * of x whose rank is the level's (0: none); clade(x) = direct_reads summed over x's subtree.  Taxa of the level with clade >=
 * max(threshold, 1) are kept; the others' clade reads are reads_below_threshold.  For every node n != 0 in ascending id with
 * direct_reads[n] > 0 and lvl(n) == 0, and every kept s in ascending id: m = sum over the genomes g with lvl(g) == s of
 * windows(g -> n), T = sum over those genomes of total(g), w(s) = m / T * clade(s) in doubles in this order (0 when T is 0).  When
 * the sum of w is positive, added(s) += direct_reads[n] * w(s) / sum; else direct_reads[n] goes to reads_undistributed.
 * new_est(s) = floor(clade(s) + added(s) + 0.5); fraction = new_est(s) / sum of new_est.  rows: one per kept taxon in ascending
 * internal id, room for n_nodes. */
typedef struct sh_k2_bracken_row { uint32_t taxon, pad; uint64_t assigned, new_est; double added, fraction; } sh_k2_bracken_row;
typedef struct sh_k2_bracken_summary {
    uint64_t n_rows;
    uint64_t reads_total;           /* sum of direct_reads */
    uint64_t reads_at_level;        /* clade reads of the kept taxa */
    uint64_t reads_below_threshold; /* clade reads of the level's other taxa */
    uint64_t reads_distributed, reads_undistributed;       /* direct reads of the nodes above the level */
    uint64_t new_est_total;
} sh_k2_bracken_summary;
sh_status sh_k2_bracken_estimate(const sh_k2_taxnode *nodes, uint64_t n_nodes, const char *ranks, uint64_t ranks_len, const uint64_t *direct_reads,
                                 const sh_k2_distrib_entry *entries, uint64_t n, const uint64_t *totals, int32_t level, uint64_t threshold,
                                 sh_k2_bracken_row *rows, sh_k2_bracken_summary *summary);
/* the table: name, taxonomy_id, taxonomy_lvl, kraken_assigned_reads, added_reads (new_est - assigned), new_est_reads,
 * fraction_total_reads (%.5f); tab-separated with a header row, rows in ascending external taxid.  path NULL or "-" = stdout */
sh_status sh_k2_bracken_write(const sh_k2_taxnode *nodes, uint64_t n_nodes, const char *names, uint64_t names_len, const sh_k2_bracken_row *rows,
                              uint64_t n_rows, int32_t level, const char *path);

/* `scrubby-hip k2-bracken-build`: the distribution of one database and one read length over library FASTA files (plain, gzip, bzip2,
 * xz), streamed in batches as sh_k2_build_run does (a record beyond chunk_bytes is cut with read_len - 1 bases repeated).  A record's
 * taxon: the header rule of sh_k2_taxonomy_header_taxon over the database's own taxonomy (seqid2taxid and / or kraken:taxid|n), or
 * `taxid` for every record; records without a taxon in the database are skipped and counted. */
typedef struct sh_k2_distrib_config {
    const char *db;                 /* database directory */
    const char *const *input;  uint32_t n_input;
    int32_t     read_len;
    const char *seqid2taxid;        /* nullable */
    uint64_t    taxid;              /* != 0: every record's (external) taxon */
    const char *output;             /* NULL: <db>/database<L>mers.kmer_distrib */
    uint64_t    chunk_bytes;        /* bases per batch, 0: 256 MiB */
    int32_t     device, pad;
} sh_k2_distrib_config;
typedef struct sh_k2_distrib_result {
    uint64_t n_records, n_skipped, n_bases, n_batches, n_cuts;
    uint64_t n_windows, n_items, n_big, n_entries;
    double   s_open, s_gpu, s_read, s_write, s_total;
} sh_k2_distrib_result;
sh_status sh_k2_distrib_run(const sh_k2_distrib_config *cfg, sh_k2_distrib_result *out);
/* `scrubby-hip k2-bracken`: re-estimates one sample from its kraken.report (as sh_k2_write_report writes it; rows are matched by
 * the taxid column, a taxid the database lacks is named once and its direct reads count as undistributed).  The taxonomy is the
 * database's (taxo.k2d is read on the host: no GPU). */
typedef struct sh_k2_bracken_config {
    const char *db;                 /* database directory */
    const char *report;             /* kraken.report */
    int32_t     read_len;           /* names the default distribution file */
    int32_t     level;              /* 0: 'S' */
    int64_t     threshold;          /* < 0: 10 */
    const char *kmer_distrib;       /* NULL: <db>/database<L>mers.kmer_distrib */
    const char *output;
} sh_k2_bracken_config;
typedef struct sh_k2_bracken_result {
    sh_k2_bracken_summary summary;
    uint64_t n_report_rows, n_unknown_taxa;
} sh_k2_bracken_result;
sh_status sh_k2_bracken_run(const sh_k2_bracken_config *cfg, sh_k2_bracken_result *out);

/* ---- DEFLATE on the device (sh_deflate.hip): the encoder behind .gz outputs when SCRUBBY_HIP_GZ_DEVICE=1 ----
 * The input is cut into blocks of block_bytes (1024..65535; 0: 32768), each compressed on its own - no match reaches before its
 * block's first byte - and written as one RFC 1951 block that starts on a byte boundary: dynamic Huffman, or stored when that is no
 * larger, so the stream is never larger than n + 5 * max(1, ceil(n / block_bytes)): the bound.  n == 0 gives the two bytes 03 00.
 * The output is the same bytes from run to run. */
typedef struct sh_deflater sh_deflater;        /* scratch for inputs of up to max_bytes at one block size; one call at a time */
typedef struct sh_deflate_stats { uint64_t n_blocks, n_stored, n_matches, n_literals, out_bytes; float ms; } sh_deflate_stats;
#define SH_DEFLATE_LITERALS_ONLY 1             /* flags bit 0: no matches, Huffman coding only */
uint64_t  sh_deflate_bound(uint64_t n, uint32_t block_bytes);
sh_status sh_deflater_create(int32_t device, uint64_t max_bytes, uint32_t block_bytes, sh_deflater **out);
/* raw DEFLATE stream; device pointers; d_in at any alignment; *out_len valid after the call (one synchronisation).
 * out_cap below the bound, or n above max_bytes: SH_ERR_BAD_ARG naming the sizes. */
sh_status sh_deflate_device(sh_deflater *df, const uint8_t *d_in, uint64_t n, int32_t flags, uint8_t *d_out, uint64_t out_cap,
                            uint64_t *out_len, void *stream, sh_deflate_stats *stats);
/* one complete gzip member from host memory: staged up through pinned memory, deflated, staged down, 10-byte header (1f 8b 08 00,
 * mtime 0, xfl 0, os 3), CRC-32 (zlib's crc32 on the host) and ISIZE.  out_cap: the bound + 18. */
sh_status sh_gzip_member(sh_deflater *df, const uint8_t *in, uint64_t n, int32_t flags, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                         sh_deflate_stats *stats);
sh_status sh_deflater_free(sh_deflater *df);

/* ---- BGZF inflate on the device (sh_inflate.hip): the decoder behind .gz inputs when SCRUBBY_HIP_GUNZIP_DEVICE=1 ----
 * A BGZF file (what bgzip writes) is a chain of gzip members of at most 64 KiB, each with its own compressed size in a BC extra
 * subfield and no reference to anything before itself.  One wave inflates one member: stored, fixed and dynamic blocks, any number per
 * member; every read stays inside the member's input extent, every write inside its ISIZE bytes, every distance inside what the member
 * has produced.  CRC-32 of the output is taken on the device and compared with the trailer's.
 * A member's status: 0 ok, 1 bad block type, 2 bad code lengths, 3 invalid symbol, 4 distance too far back, 5 input overrun,
 * 6 output overrun, 7 output short of ISIZE, 8 stored LEN/NLEN mismatch, 9 CRC mismatch. */
typedef struct sh_gz_member { uint64_t file_off, in_off; uint32_t in_len, out_len, crc32, status; } sh_gz_member;
typedef struct sh_inflater sh_inflater;        /* scratch for calls of up to max_members members; one call at a time */
typedef struct sh_inflate_stats { uint64_t n_members, n_stored_blocks, n_fixed_blocks, n_dynamic_blocks, in_bytes, out_bytes; float ms; } sh_inflate_stats;
/* host only: the members of buf[0, n), a window of a file.  file_off: the member's offset in buf; in_off / in_len: its raw DEFLATE
 * data; out_len / crc32: ISIZE and CRC-32 of its trailer.  *n_members found (at most cap), *consumed = bytes of buf they cover,
 * *stopped = 0 end of buffer (or cap reached), 1 incomplete member, 2 not BGZF (not gzip, no BC subfield, ISIZE above 65536). */
sh_status sh_bgzf_scan(const uint8_t *buf, uint64_t n, sh_gz_member *members, uint64_t cap, uint64_t *n_members, uint64_t *consumed, int32_t *stopped);
sh_status sh_inflater_create(int32_t device, uint64_t max_in_bytes, uint64_t max_out_bytes, uint64_t max_members, sh_inflater **out);
/* device pointers; members on the host, in any order: member i's bytes go to d_out + the sum of out_len before it, its data is
 * d_in[in_off, in_off + in_len), and its status is filled on return (one synchronisation).  SH_ERR_IO names the first bad member's
 * file_off and status.  More members, an input extent or an output larger than the inflater was made for, or out_cap below the sum of
 * out_len: SH_ERR_BAD_ARG naming the sizes, before any launch. */
sh_status sh_inflate_members_device(sh_inflater *inf, const uint8_t *d_in, sh_gz_member *members, uint64_t n_members, uint8_t *d_out, uint64_t out_cap,
                                    void *stream, sh_inflate_stats *stats);
/* host memory in and out through pinned staging: scan + inflate of a buffer that holds whole members only (else SH_ERR_IO naming
 * the offset where the scan stopped) */
sh_status sh_gunzip_bgzf(sh_inflater *inf, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_len, sh_inflate_stats *stats);
sh_status sh_inflater_free(sh_inflater *inf);

/* ---- any gzip stream on the device (sh_gunzip_*): what gzip, pigz or a sequencer writes, one long member as well as many ----
 * The window of compressed bytes a feed is given is cut into chunks of chunk_bytes at fixed offsets.  k_gz_find looks for a DEFLATE
 * block start in every chunk, k_gz_size decodes from each start to the first block boundary past the chunk's end and counts, the host
 * walks the chain of end bits (a chunk that does not start where its predecessor ended is decoded again from there, at most 8 rounds),
 * k_gz_markers decodes the chain's spans once more to 16-bit symbols in which a reference to the 32 KiB before the span is a marker,
 * k_gz_tails settles the windows behind spans whose last 32 KiB hold no marker, k_gz_windows passes the 32 KiB along the rest of the
 * chain and k_gz_resolve replaces the markers and takes the CRC-32 in pieces.
 * A feed
 *   - decodes as many whole chunks as out_cap (and the inflater's max_out_bytes) holds; *consumed is the count of whole input bytes the
 *     caller may drop: it presents the rest again, in front of new bytes.  n may not exceed the inflater's max_in_bytes;
 *   - with last != 0 wants the stream to end at a member end (what follows a member and is no gzip member is ignored, as gzread
 *     ignores it), else SH_ERR_IO naming the file offset;
 *   - returns SH_ERR_BAD_ARG naming the size when out_cap is below what the first chunk needs;
 *   - returns SH_ERR_IO with the member's file offset and the status for data that does not decode, a CRC-32 or ISIZE (modulo 2^32)
 *     that does not hold, or a distance too far back: never a short or wrong output;
 *   - returns SH_GUNZIP_FALLBACK when 8 rounds leave a chunk open (a stream of fixed blocks has no block start to find) or more than
 *     four members end in one chunk's span: *consumed and *out_len then cover what was decoded before, which is right, and the
 *     caller reads the file another way.
 * After any status but SH_OK the sh_gunzip takes no further feed.  One call at a time per inflater; sh_gunzip_close before
 * sh_inflater_free.  The scratch (2 B per byte of max_out_bytes, 32 KiB per chunk of max_in_bytes) is the inflater's and is allocated
 * by the first sh_gunzip_open, so an inflater that only sees BGZF takes what it took before. */
#define SH_GUNZIP_FALLBACK 10
typedef struct sh_gunzip sh_gunzip;   /* one gzip file being read: resume bit, last 32 KiB of output, the open member's CRC-32 and length so far */
typedef struct sh_gunzip_stats { uint64_t n_chunks, n_skipped, n_redone, n_rounds, n_members, n_marker_symbols, n_window_steps, in_bytes, out_bytes;
                                 float ms_find, ms_size, ms_markers, ms_windows, ms_resolve, ms; } sh_gunzip_stats;
sh_status sh_gunzip_open(sh_inflater *inf, uint32_t chunk_bytes /* 1 KiB .. 1 MiB, 0: the default */, sh_gunzip **out);
sh_status sh_gunzip_feed_device(sh_gunzip *gz, const uint8_t *d_in, uint64_t n, int32_t last, uint8_t *d_out, uint64_t out_cap,
                                uint64_t *consumed, uint64_t *out_len, void *stream, sh_gunzip_stats *stats);
sh_status sh_gunzip_feed(sh_gunzip *gz, const uint8_t *in, uint64_t n, int32_t last, uint8_t *out, uint64_t out_cap,
                         uint64_t *consumed, uint64_t *out_len, sh_gunzip_stats *stats);      /* host memory through the inflater's pinned staging */
sh_status sh_gunzip_close(sh_gunzip *gz);
/* test aid: one feed (last != 0) of a whole stream in HBM in which the caller names the chunk starts instead of k_gz_find: starts[j],
 * j >= 1, is a bit position of the stream or ~0 for none (n_starts = the number of chunks, else SH_ERR_BAD_ARG); a start outside its
 * chunk counts as none.  Wrong starts cost rounds, never bytes. */
sh_status sh_dbg_gunzip_starts(sh_inflater *inf, uint32_t chunk_bytes, const uint8_t *d_in, uint64_t n, const uint64_t *starts, uint64_t n_starts,
                               uint8_t *d_out, uint64_t out_cap, uint64_t *out_len, void *stream, sh_gunzip_stats *stats);

/* ---- BAM records filtered on the device (sh_bam.hip): the reader behind `scrubby alignment -a x.bam` when
 *      SCRUBBY_HIP_GUNZIP_DEVICE is 1 or 2 ----
 * The rule (ReadAlignment::from_bam, alignment.rs:115-211): for every record that is not unmapped (flag & 4), qalen = the lengths of
 * its CIGAR ops M and I (= and X count nothing), summed in 64 bits; qlen = l_seq; qcov = qlen ? (double)qalen / (double)qlen : 0; the
 * record's name is selected iff (qalen >= min_len || qcov >= min_cov) && mapq >= min_mapq.  A name is the l_read_name - 1 bytes
 * before the terminating NUL, compared as bytes (the reference's UTF-8 check is not reproduced).  The CIGAR is the CG:B,I tag's when
 * n_cigar_op != 0, refID >= 0, pos >= 0, the first stored op is <l_seq>S and the record's first CG tag is B,I with a count
 * >= n_cigar_op and < 2^29 (htslib's bam_tag2cigar as recalled: PARITY WITH htslib UNPINNED); else the stored one.
 * A record may start at p when (judged on the bytes of it that lie in the window) block_size is in [32 + l_read_name + 4 * n_cigar_op
 * + (l_seq + 1) / 2 + l_seq, 64 MiB] with l_seq >= 0, l_read_name >= 1, the name's last byte is 0, refID and next_refID lie in
 * [-1, n_ref), pos and next_pos are >= -1.
 *
 * text[0, n) is a window of the inflated record stream; base its offset in the stream (for error messages only); entry the offset in
 * the window of a record start.  Out: the names of the selected records, each followed by one NUL, in record order (duplicates stay),
 * and *next_entry, the first chain position whose record does not lie in the window whole: the caller presents the bytes from there
 * again, in front of new ones.  With last != 0 the chain must end at n, else SH_ERR_IO "truncated BAM record at <base + p>"; a chain
 * position that is no record is SH_ERR_IO "not a BAM record at <base + p>": never a short or wrong output.  names_cap below
 * sh_bam_names_bound(n - entry), or n above the scanner's size: SH_ERR_BAD_ARG naming the sizes, before any launch.
 * stats: n_segments counts the segments (of sh_bam_segment() bytes, at fixed offsets of the window) in which a record of the chain
 * starts; n_plausible the positions at which a record may start and n_fallback_segments the segments walked on the host because they
 * hold more such positions than sh_bam_segment_cap() are the device path's (0 from the host). */
typedef struct sh_bam_rule  { uint64_t min_len; double min_cov; uint32_t min_mapq; int32_t n_ref; } sh_bam_rule;
typedef struct sh_bam_stats { uint64_t n_records, n_unmapped, n_selected, n_cg, n_segments, n_plausible, n_fallback_segments, name_bytes;
                              float ms_probe, ms_chain, ms_filter, ms; } sh_bam_stats;
typedef struct sh_bam_scanner sh_bam_scanner;  /* scratch for windows of up to max_bytes (below 2^31); one call at a time */
/* host only: the header of text[0, n).  *stopped = 0: *n_ref and *first_record (the offset of the first record) are set; 1: needs more
 * bytes; 2: not BAM */
sh_status sh_bam_header(const uint8_t *text, uint64_t n, int32_t *n_ref, uint64_t *first_record, int32_t *stopped);
uint32_t  sh_bam_segment(void);      /* bytes per segment */
uint32_t  sh_bam_segment_cap(void);  /* plausible starts a segment's table holds */
uint64_t  sh_bam_names_bound(uint64_t n);      /* the most name bytes n bytes of records give */
sh_status sh_bam_scanner_create(int32_t device, uint64_t max_bytes, sh_bam_scanner **out);
sh_status sh_bam_scanner_free(sh_bam_scanner *sc);
sh_status sh_bam_filter_device(sh_bam_scanner *sc, const uint8_t *d_text, uint64_t n, uint64_t base, uint64_t entry, int32_t last, const sh_bam_rule *rule,
                               uint8_t *d_names, uint64_t names_cap, uint64_t *names_len, uint64_t *next_entry, void *stream, sh_bam_stats *stats);
/* the host mirror (no GPU): the same answer from the same code (sh_bam.h) in one serial walk */
sh_status sh_bam_filter_host(const uint8_t *text, uint64_t n, uint64_t base, uint64_t entry, int32_t last, const sh_bam_rule *rule, uint8_t *names, uint64_t names_cap,
                             uint64_t *names_len, uint64_t *next_entry, sh_bam_stats *stats);
/* host only, for the tests of the table's size: counts[s] = the positions of segment s at which a record may start */
sh_status sh_bam_plausible_host(const uint8_t *text, uint64_t n, int32_t n_ref, uint32_t *counts, uint64_t n_counts);

#ifdef __cplusplus
}
#endif
#endif
