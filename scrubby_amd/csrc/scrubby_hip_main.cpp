// scrubby-hip — command-line front end of the replaced path, with the flags of `scrubby reads`
// (/root/reference/src/terminal.rs:57-157).  Only what the mm2 aligner path uses is implemented; options that
// select other aligners / classifiers are accepted and rejected with the reason.
#include "../../include/scrubby_hip.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static void usage()
{
    fprintf(stderr,
            "scrubby-hip reads -i <R1> [R2] -o <O1> [O2] -I <ref.fa[.gz]|index.shidx> [-p sr|map-ont|lr:hq|map-hifi]\n"
            "                  [-e] [-j report.json] [-r read_ids.tsv[.gz]] [-t threads] [-a minimap2-rs] [-w workdir]\n"
            "scrubby-hip reads -i <R1> [R2] -o <O1> [O2] -c kraken2 -I <kraken2 db dir> [-T taxa..] [-D taxa..] [-w workdir]\n"
            "                  [-C \"--confidence x --minimum-hit-groups n\"] [-e] [-j report.json] [-r read_ids.tsv[.gz]]\n"
            "scrubby-hip classifier -i <R1> [R2] -o <O1> [O2] -k <report> -j <reads> -c kraken2|metabuli [-T taxa..] [-D taxa..]\n"
            "                  [-e] [--json report.json] [-r read_ids.tsv]\n"
            "scrubby-hip k2-build -i <library.fna[.gz]>.. -o <db dir> (-n <taxonomy dir> [-m <seqid2taxid.map>] | --taxid N [--name S] [--rank S])\n"
            "                  [--kmer-len 35] [--minimizer-len 31] [--minimizer-spaces 7] [--capacity N] [--load-factor 0.7]\n"
            "                  [--max-db-size BYTES] [--value-bits N] [--chunk-bytes N]\n"
            "                  [--mask-low-complexity [--mask-window 64] [--mask-threshold 20]]\n"
            "                  [--protein]   (an amino-acid FASTA library: k 15, l 12, no minimizer spaces; reads are then searched in\n"
            "                                 six translated frames; no --mask-low-complexity, --quick, hit lists or minimizer data)\n"
            "scrubby-hip k2-mask -i <in.fa[.gz|.bz2|.xz]> -o <out.fa[.gz|.bz2|.xz]> [-W 64] [-T 20] [-r x | --soft] [--line-width 60]\n"
            "                  [--chunk-bytes N]\n"
            "scrubby-hip k2-inspect -d <db dir> [-o report.txt] [--skip-counts] [--report-zero-counts] [--use-mpa-style] [--device N]\n"
            "scrubby-hip k2-bracken-build -d <db dir> -i <library.fna[.gz]>.. [-m <seqid2taxid.map> | --taxid N] -l <read length> [-o FILE]\n"
            "                  [--chunk-bytes N] [--device N]\n"
            "scrubby-hip k2-bracken -d <db dir> -r <kraken.report> -l <read length> [-L S] [-t 10] [-k <kmer_distrib>] -o <sample.bracken>\n");
}

// `scrubby classifier` (/root/reference/src/terminal.rs:204-279): clean reads from precomputed Kraken2 / Metabuli outputs
static int main_classifier(int argc, char **argv, const std::string &command)
{
    std::vector<std::string> in, out, taxa, direct;
    std::string report, reads, classifier, json, ids;
    int extract = 0;
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) { fprintf(stderr, "missing value for %s\n", a.c_str()); exit(2); } return argv[++i]; };
        auto multi = [&](std::vector<std::string> &v) { while (i + 1 < argc && argv[i + 1][0] != '-') v.push_back(argv[++i]); };
        if (a == "-i" || a == "--input") multi(in);
        else if (a == "-o" || a == "--output") multi(out);
        else if (a == "-k" || a == "--report") report = val();
        else if (a == "-j" || a == "--reads") reads = val();          // the reference binds -j to --reads AND --json (App. C Q13): --json has no short here
        else if (a == "-c" || a == "--classifier") classifier = val();
        else if (a == "-T" || a == "--taxa") multi(taxa);
        else if (a == "-D" || a == "--taxa-direct") multi(direct);
        else if (a == "--json") json = val();
        else if (a == "-r" || a == "--read-ids") ids = val();
        else if (a == "-w" || a == "--workdir") val();
        else if (a == "-e" || a == "--extract") extract = 1;
        else { fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }
    if (in.empty() || in.size() > 2 || in.size() != out.size()) { fprintf(stderr, "error: one or two inputs and as many outputs are required\n"); return 2; }
    std::vector<const char *> tp, dp;
    for (auto &t : taxa) tp.push_back(t.c_str());
    for (auto &t : direct) dp.push_back(t.c_str());
    sh_classifier_config c{};
    for (size_t k = 0; k < in.size(); ++k) { c.input[k] = in[k].c_str(); c.output[k] = out[k].c_str(); }
    c.n_files = (uint32_t)in.size(); c.extract = extract;
    c.report = report.empty() ? nullptr : report.c_str(); c.reads = reads.empty() ? nullptr : reads.c_str();
    c.classifier = classifier.empty() ? nullptr : classifier.c_str();
    c.taxa = tp.data(); c.n_taxa = (uint32_t)tp.size(); c.taxa_direct = dp.data(); c.n_taxa_direct = (uint32_t)dp.size();
    c.json = json.empty() ? nullptr : json.c_str(); c.read_ids = ids.empty() ? nullptr : ids.c_str(); c.command = command.c_str();
    sh_reads_result r{};
    sh_status st = sh_classifier_run(&c, &r);
    if (st != SH_OK) { fprintf(stderr, "error (%d): %s\n", st, sh_last_error()); return 1; }
    fprintf(stderr, "[scrubby-hip] read ids selected by taxid: %llu\n", (unsigned long long)r.n_depleted_ids);
    return 0;
}

// `scrubby-hip k2-build`: a Kraken 2 database directory from a FASTA library and a taxonomy (no counterpart in the reference, which
// takes a finished database; kraken2-build's options)
static int main_k2_build(int argc, char **argv)
{
    std::vector<std::string> in;
    std::string out, taxdir, map, name, rank;
    sh_k2_build_config c{};
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) { fprintf(stderr, "missing value for %s\n", a.c_str()); exit(2); } return argv[++i]; };
        auto multi = [&](std::vector<std::string> &v) { while (i + 1 < argc && argv[i + 1][0] != '-') v.push_back(argv[++i]); };
        if (a == "-i" || a == "--input") multi(in);
        else if (a == "-o" || a == "--output") out = val();
        else if (a == "-n" || a == "--taxonomy") taxdir = val();
        else if (a == "-m" || a == "--seqid2taxid") map = val();
        else if (a == "--taxid") c.taxid = strtoull(val().c_str(), nullptr, 10);
        else if (a == "--name") name = val();
        else if (a == "--rank") rank = val();
        else if (a == "--kmer-len") c.k = atoi(val().c_str());
        else if (a == "--minimizer-len") c.l = atoi(val().c_str());
        else if (a == "--minimizer-spaces") { c.minimizer_spaces = atoi(val().c_str()); if (c.minimizer_spaces == 0) c.minimizer_spaces = -1; }
        else if (a == "--capacity") c.capacity = strtoull(val().c_str(), nullptr, 10);
        else if (a == "--load-factor") c.load_factor = atof(val().c_str());
        else if (a == "--max-db-size") c.max_db_size = strtoull(val().c_str(), nullptr, 10);
        else if (a == "--value-bits") c.value_bits = atoi(val().c_str());
        else if (a == "--chunk-bytes") c.chunk_bytes = strtoull(val().c_str(), nullptr, 10);
        else if (a == "--mask-low-complexity") c.mask_low_complexity = 1;
        else if (a == "--protein") c.protein = 1;
        else if (a == "--mask-window") c.mask_window = atoi(val().c_str());
        else if (a == "--mask-threshold") c.mask_threshold = atoi(val().c_str());
        else { fprintf(stderr, "unknown argument %s\n", a.c_str()); usage(); return 2; }
    }
    if (in.empty() || out.empty()) { fprintf(stderr, "error: library files (-i) and an output directory (-o) are required\n"); return 2; }
    if (taxdir.empty() == (c.taxid == 0)) { fprintf(stderr, "error: either -n <taxonomy dir> or --taxid N\n"); return 2; }
    std::vector<const char *> ip;
    for (auto &x : in) ip.push_back(x.c_str());
    c.input = ip.data(); c.n_input = (uint32_t)ip.size(); c.output_dir = out.c_str();
    c.taxonomy_dir = taxdir.empty() ? nullptr : taxdir.c_str(); c.seqid2taxid = map.empty() ? nullptr : map.c_str();
    c.name = name.empty() ? nullptr : name.c_str(); c.rank = rank.empty() ? nullptr : rank.c_str();
    sh_k2_build_result r{};
    sh_status st = sh_k2_build_run(&c, &r);
    if (st != SH_OK) { fprintf(stderr, "error (%d): %s\n", st, sh_last_error()); return 1; }
    printf("{\"records\": %llu, \"records_skipped\": %llu, \"bases\": %llu, \"batches\": %llu, \"cuts\": %llu, \"runs_inserted\": %llu, \"size\": %llu, "
           "\"capacity\": %llu, \"nodes\": %llu, \"value_bits\": %d, \"n_sampled\": %llu, \"estimate\": %llu, \"min_acceptable_hash\": %llu, "
           "\"s_estimate\": %.3f, \"s_taxonomy\": %.3f, \"s_fill\": %.3f, \"s_save\": %.3f, \"s_read\": %.3f, \"s_total\": %.3f",
           (unsigned long long)r.n_records, (unsigned long long)r.n_skipped, (unsigned long long)r.n_bases, (unsigned long long)r.n_batches,
           (unsigned long long)r.n_cuts, (unsigned long long)r.n_runs, (unsigned long long)r.size, (unsigned long long)r.capacity, (unsigned long long)r.n_nodes,
           r.value_bits, (unsigned long long)r.n_sampled, (unsigned long long)r.estimate, (unsigned long long)r.min_acceptable_hash, r.s_estimate, r.s_taxonomy,
           r.s_fill, r.s_save, r.s_read, r.s_total);
    if (c.mask_low_complexity) printf(", \"masked_bases\": %llu, \"s_mask\": %.3f", (unsigned long long)r.n_masked_bases, r.s_mask);      // only with the flag
    printf("}\n");
    return 0;
}

// `scrubby-hip k2-mask`: the masking step of a build on its own, FASTA to FASTA (what running k2mask by hand gives kraken2-build)
static int main_k2_mask(int argc, char **argv)
{
    std::string in, out;
    sh_k2_mask_config c{};
    c.line_width = 60;
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) { fprintf(stderr, "missing value for %s\n", a.c_str()); exit(2); } return argv[++i]; };
        if (a == "-i" || a == "--input") in = val();
        else if (a == "-o" || a == "--output") out = val();
        else if (a == "-W" || a == "--window") c.window = atoi(val().c_str());
        else if (a == "-T" || a == "--threshold") c.threshold = atoi(val().c_str());
        else if (a == "-r" || a == "--replacement") { const std::string v = val(); if (v.size() != 1) { fprintf(stderr, "error: -r takes one character\n"); return 2; } c.replacement = (unsigned char)v[0]; }
        else if (a == "--soft") c.soft = 1;
        else if (a == "--line-width") c.line_width = atoi(val().c_str());
        else if (a == "--chunk-bytes") c.chunk_bytes = strtoull(val().c_str(), nullptr, 10);
        else { fprintf(stderr, "unknown argument %s\n", a.c_str()); usage(); return 2; }
    }
    if (in.empty() || out.empty()) { fprintf(stderr, "error: an input (-i) and an output (-o) FASTA file are required\n"); return 2; }
    if (c.soft && c.replacement) { fprintf(stderr, "error: either -r or --soft\n"); return 2; }
    c.input = in.c_str(); c.output = out.c_str();
    sh_k2_mask_result r{};
    sh_status st = sh_k2_mask_run(&c, &r);
    if (st != SH_OK) { fprintf(stderr, "error (%d): %s\n", st, sh_last_error()); return 1; }
    printf("{\"records\": %llu, \"bases\": %llu, \"masked_bases\": %llu, \"batches\": %llu, \"cuts\": %llu, \"s_mask\": %.3f, \"s_total\": %.3f}\n",
           (unsigned long long)r.n_records, (unsigned long long)r.n_bases, (unsigned long long)r.n_masked_bases, (unsigned long long)r.n_batches,
           (unsigned long long)r.n_cuts, r.s_mask, r.s_total);
    return 0;
}

// `scrubby-hip k2-inspect`: the options a database was built with and its minimizers per taxon (kraken2-inspect's options)
static int main_k2_inspect(int argc, char **argv)
{
    std::string db, out;
    sh_k2_inspect_config c{};
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) { fprintf(stderr, "missing value for %s\n", a.c_str()); exit(2); } return argv[++i]; };
        if (a == "-d" || a == "--db") db = val();
        else if (a == "-o" || a == "--output") out = val();
        else if (a == "--skip-counts") c.skip_counts = 1;
        else if (a == "--report-zero-counts") c.report_zero_counts = 1;
        else if (a == "--use-mpa-style") c.use_mpa_style = 1;
        else if (a == "--device") c.device = atoi(val().c_str());
        else { fprintf(stderr, "unknown argument %s\n", a.c_str()); usage(); return 2; }
    }
    if (db.empty()) { fprintf(stderr, "error: a database directory (-d) is required\n"); return 2; }
    c.db = db.c_str(); c.output = out.empty() ? nullptr : out.c_str();
    sh_k2_inspect_result r{};
    sh_status st = sh_k2_inspect_run(&c, &r);
    if (st != SH_OK) { fprintf(stderr, "error (%d): %s\n", st, sh_last_error()); return 1; }
    // the report may be on stdout: the figures go to stderr
    fprintf(stderr, "[scrubby-hip] capacity %llu, size %llu, occupied %llu, nodes %llu, taxa with minimizers %llu; open %.3f s, count %.3f s, report %.3f s, total %.3f s\n",
            (unsigned long long)r.capacity, (unsigned long long)r.size_header, (unsigned long long)r.n_occupied, (unsigned long long)r.n_nodes,
            (unsigned long long)r.n_taxa_with_minimizers, r.s_open, r.s_count, r.s_report, r.s_total);
    return 0;
}

// `scrubby-hip k2-bracken-build`: bracken-build's k-mer distribution of a database at one read length, on the GPU
static int main_k2_bracken_build(int argc, char **argv)
{
    std::vector<std::string> in;
    std::string db, map, out;
    sh_k2_distrib_config c{};
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) { fprintf(stderr, "missing value for %s\n", a.c_str()); exit(2); } return argv[++i]; };
        auto multi = [&](std::vector<std::string> &v) { while (i + 1 < argc && argv[i + 1][0] != '-') v.push_back(argv[++i]); };
        if (a == "-d" || a == "--db") db = val();
        else if (a == "-i" || a == "--input") multi(in);
        else if (a == "-m" || a == "--seqid2taxid") map = val();
        else if (a == "--taxid") c.taxid = strtoull(val().c_str(), nullptr, 10);
        else if (a == "-l" || a == "--read-len") c.read_len = atoi(val().c_str());
        else if (a == "-o" || a == "--output") out = val();
        else if (a == "--chunk-bytes") c.chunk_bytes = strtoull(val().c_str(), nullptr, 10);
        else if (a == "--device") c.device = atoi(val().c_str());
        else { fprintf(stderr, "unknown argument %s\n", a.c_str()); usage(); return 2; }
    }
    if (db.empty() || in.empty() || c.read_len <= 0) { fprintf(stderr, "error: a database directory (-d), library files (-i) and a read length (-l) are required\n"); usage(); return 2; }
    std::vector<const char *> ip;
    for (auto &f : in) ip.push_back(f.c_str());
    c.db = db.c_str(); c.input = ip.data(); c.n_input = (uint32_t)ip.size();
    c.seqid2taxid = map.empty() ? nullptr : map.c_str(); c.output = out.empty() ? nullptr : out.c_str();
    sh_k2_distrib_result r{};
    sh_status st = sh_k2_distrib_run(&c, &r);
    if (st != SH_OK) { fprintf(stderr, "error (%d): %s\n", st, sh_last_error()); return 1; }
    fprintf(stderr, "[scrubby-hip] %llu records (%llu skipped), %llu bases, %llu batches (%llu cuts): %llu windows, %llu stretches (%llu redone), %llu entries; "
            "open %.3f s, gpu %.3f s, read %.3f s, total %.3f s\n",
            (unsigned long long)r.n_records, (unsigned long long)r.n_skipped, (unsigned long long)r.n_bases, (unsigned long long)r.n_batches, (unsigned long long)r.n_cuts,
            (unsigned long long)r.n_windows, (unsigned long long)r.n_items, (unsigned long long)r.n_big, (unsigned long long)r.n_entries, r.s_open, r.s_gpu, r.s_read, r.s_total);
    return 0;
}

// `scrubby-hip k2-bracken`: Bracken's abundance estimate of one sample from its kraken.report (host only)
static int main_k2_bracken(int argc, char **argv)
{
    std::string db, report, dist, out;
    sh_k2_bracken_config c{};
    c.threshold = -1;
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) { fprintf(stderr, "missing value for %s\n", a.c_str()); exit(2); } return argv[++i]; };
        if (a == "-d" || a == "--db") db = val();
        else if (a == "-r" || a == "--report") report = val();
        else if (a == "-l" || a == "--read-len") c.read_len = atoi(val().c_str());
        else if (a == "-L" || a == "--level") { const std::string v = val(); c.level = v.size() == 1 ? v[0] : '?'; }
        else if (a == "-t" || a == "--threshold") c.threshold = atoll(val().c_str());
        else if (a == "-k" || a == "--kmer-distrib") dist = val();
        else if (a == "-o" || a == "--output") out = val();
        else { fprintf(stderr, "unknown argument %s\n", a.c_str()); usage(); return 2; }
    }
    if (db.empty() || report.empty() || out.empty() || (dist.empty() && c.read_len <= 0)) {
        fprintf(stderr, "error: a database directory (-d), a report (-r), a read length (-l) or a distribution file (-k), and an output (-o) are required\n");
        usage();
        return 2;
    }
    c.db = db.c_str(); c.report = report.c_str(); c.output = out.c_str(); c.kmer_distrib = dist.empty() ? nullptr : dist.c_str();
    sh_k2_bracken_result r{};
    sh_status st = sh_k2_bracken_run(&c, &r);
    if (st != SH_OK) { fprintf(stderr, "error (%d): %s\n", st, sh_last_error()); return 1; }
    fprintf(stderr, "[scrubby-hip] %llu taxa at the level: %llu reads there, %llu below the threshold, %llu distributed, %llu undistributed; new estimate %llu reads\n",
            (unsigned long long)r.summary.n_rows, (unsigned long long)r.summary.reads_at_level, (unsigned long long)r.summary.reads_below_threshold,
            (unsigned long long)r.summary.reads_distributed, (unsigned long long)r.summary.reads_undistributed, (unsigned long long)r.summary.new_est_total);
    return 0;
}

// `scrubby alignment` (/root/reference/src/terminal.rs:281-360)
static int main_alignment(int argc, char **argv, const std::string &command)
{
    std::vector<std::string> in, out;
    std::string aln, fmt, json, ids;
    unsigned long long min_len = 0; double min_cov = 0.0; unsigned min_mapq = 0;
    int extract = 0;
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) { fprintf(stderr, "missing value for %s\n", a.c_str()); exit(2); } return argv[++i]; };
        auto multi = [&](std::vector<std::string> &v) { while (i + 1 < argc && argv[i + 1][0] != '-') v.push_back(argv[++i]); };
        if (a == "-i" || a == "--input") multi(in);
        else if (a == "-o" || a == "--output") multi(out);
        else if (a == "-a" || a == "--alignment") aln = val();
        else if (a == "-f" || a == "--format") fmt = val();
        else if (a == "-l" || a == "--min-len") min_len = strtoull(val().c_str(), nullptr, 10);
        else if (a == "-c" || a == "--min-cov") min_cov = atof(val().c_str());
        else if (a == "-q" || a == "--min-mapq") min_mapq = (unsigned)atoi(val().c_str());
        else if (a == "-j" || a == "--json") json = val();
        else if (a == "-r" || a == "--read-ids") ids = val();
        else if (a == "-w" || a == "--workdir") val();
        else if (a == "-e" || a == "--extract") extract = 1;
        else { fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }
    if (in.empty() || in.size() > 2 || in.size() != out.size()) { fprintf(stderr, "error: one or two inputs and as many outputs are required\n"); return 2; }
    sh_alignment_config c{};
    for (size_t k = 0; k < in.size(); ++k) { c.input[k] = in[k].c_str(); c.output[k] = out[k].c_str(); }
    c.n_files = (uint32_t)in.size(); c.extract = extract; c.alignment = aln.empty() ? nullptr : aln.c_str();
    c.format = fmt.empty() ? nullptr : fmt.c_str(); c.min_len = min_len; c.min_cov = min_cov; c.min_mapq = min_mapq;
    c.json = json.empty() ? nullptr : json.c_str(); c.read_ids = ids.empty() ? nullptr : ids.c_str(); c.command = command.c_str();
    sh_reads_result r{};
    sh_status st = sh_alignment_run(&c, &r);
    if (st != SH_OK) { fprintf(stderr, "error (%d): %s\n", st, sh_last_error()); return 1; }
    fprintf(stderr, "[scrubby-hip] read ids selected by alignment: %llu\n", (unsigned long long)r.n_depleted_ids);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && std::string(argv[1]) == "k2-build") return main_k2_build(argc, argv);
    if (argc >= 2 && std::string(argv[1]) == "k2-mask") return main_k2_mask(argc, argv);
    if (argc >= 2 && std::string(argv[1]) == "k2-inspect") return main_k2_inspect(argc, argv);
    if (argc >= 2 && std::string(argv[1]) == "k2-bracken-build") return main_k2_bracken_build(argc, argv);
    if (argc >= 2 && std::string(argv[1]) == "k2-bracken") return main_k2_bracken(argc, argv);
    if (argc >= 2 && (std::string(argv[1]) == "classifier" || std::string(argv[1]) == "alignment")) {
        std::string command;
        for (int i = 0; i < argc; ++i) { if (i) command += ' '; command += argv[i]; }
        return std::string(argv[1]) == "alignment" ? main_alignment(argc, argv, command) : main_classifier(argc, argv, command);
    }
    if (argc < 2 || std::string(argv[1]) != "reads") { usage(); return 2; }
    std::vector<std::string> in, out, taxa, taxa_direct;
    std::string index, preset, json, ids, aligner, classifier, workdir, cargs, command;
    int extract = 0, threads = 0;      // 0: the CPUs this process may use (the deflate stage of .gz outputs scales with them)
    for (int i = 0; i < argc; ++i) { if (i) command += ' '; command += argv[i]; }      // terminal.rs:178
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) { fprintf(stderr, "missing value for %s\n", a.c_str()); exit(2); } return argv[++i]; };
        auto multi = [&](std::vector<std::string> &v) { while (i + 1 < argc && argv[i + 1][0] != '-') v.push_back(argv[++i]); };
        if (a == "-i" || a == "--input") multi(in);
        else if (a == "-o" || a == "--output") multi(out);
        else if (a == "-I" || a == "--index") index = val();
        else if (a == "-p" || a == "--preset") preset = val();
        else if (a == "-a" || a == "--aligner") aligner = val();
        else if (a == "-c" || a == "--classifier") classifier = val();
        else if (a == "-T" || a == "--taxa") multi(taxa);
        else if (a == "-D" || a == "--taxa-direct") multi(taxa_direct);
        else if (a == "-C" || a == "--classifier-args") cargs = val();
        else if (a == "-j" || a == "--json") json = val();
        else if (a == "-r" || a == "--read-ids") ids = val();
        else if (a == "-t" || a == "--threads") threads = atoi(val().c_str());
        else if (a == "-w" || a == "--workdir") workdir = val();
        else if (a == "-l" || a == "--log-file" || a == "-A" || a == "--aligner-args") val();
        else if (a == "-e" || a == "--extract") extract = 1;
        else { fprintf(stderr, "unknown argument %s\n", a.c_str()); usage(); return 2; }
    }
    if (in.empty() || in.size() > 2 || in.size() != out.size()) { fprintf(stderr, "error: one or two inputs and as many outputs are required\n"); return 2; }
    if (!classifier.empty()) {       // Cleaner::run_classifier (cleaner.rs:159-163): kraken2 on the GPU
        if (classifier != "kraken2") { fprintf(stderr, "error: the HIP backend replaces --classifier kraken2 only (got %s)\n", classifier.c_str()); return 2; }
        if (!aligner.empty()) { fprintf(stderr, "error: AlignerAndClassifierConfigured\n"); return 2; }
        if (index.empty()) { fprintf(stderr, "error: MissingClassifierIndex (-I)\n"); return 2; }
        sh_kraken_config k{};
        std::vector<const char *> tp, dp;
        for (auto &x : taxa) tp.push_back(x.c_str());
        for (auto &x : taxa_direct) dp.push_back(x.c_str());
        for (size_t q = 0; q < in.size(); ++q) { k.input[q] = in[q].c_str(); k.output[q] = out[q].c_str(); }
        k.n_files = (uint32_t)in.size(); k.extract = extract; k.db = index.c_str(); k.workdir = workdir.empty() ? nullptr : workdir.c_str();
        k.taxa = tp.data(); k.n_taxa = (uint32_t)tp.size(); k.taxa_direct = dp.data(); k.n_taxa_direct = (uint32_t)dp.size();
        k.confidence = -1.0; k.min_hit_groups = 0;
        {   // the two Kraken 2 thresholds out of --classifier-args
            size_t p = cargs.find("--confidence");
            if (p != std::string::npos) k.confidence = atof(cargs.c_str() + p + 12);
            p = cargs.find("--minimum-hit-groups");
            if (p != std::string::npos) k.min_hit_groups = atoi(cargs.c_str() + p + 20);
        }
        {   // --minimum-base-quality n (or =n), --quick and --report-minimizer-data by tokens; any other token is named once on stderr
            std::vector<std::string> tok, ignored;
            for (size_t p = 0; (p = cargs.find_first_not_of(" \t", p)) != std::string::npos;) {
                const size_t e = std::min(cargs.find_first_of(" \t", p), cargs.size());
                tok.push_back(cargs.substr(p, e - p)); p = e;
            }
            for (size_t t = 0; t < tok.size(); ++t) {
                const std::string &x = tok[t];
                const bool has_next = t + 1 < tok.size();
                if (x == "--quick") k.quick = 1;
                else if (x == "--report-minimizer-data") k.report_minimizer_data = 1;
                else if (x == "--minimum-base-quality" && has_next) k.min_base_quality = atoi(tok[++t].c_str());
                else if (x.rfind("--minimum-base-quality=", 0) == 0) k.min_base_quality = atoi(x.c_str() + 23);
                else if ((x == "--confidence" || x == "--minimum-hit-groups") && has_next) ++t;      // read above
                else if (x.rfind("--confidence", 0) == 0 || x.rfind("--minimum-hit-groups", 0) == 0) {}
                else ignored.push_back(x);
            }
            if (!ignored.empty()) {
                std::string l;
                for (auto &x : ignored) l += " " + x;
                fprintf(stderr, "[scrubby-hip] -C: ignored by the HIP backend's kraken2:%s\n", l.c_str());
            }
        }
        k.json = json.empty() ? nullptr : json.c_str(); k.read_ids = ids.empty() ? nullptr : ids.c_str();
        k.command = command.c_str(); k.device = 0; k.threads = threads;
        k.classifier_args = cargs.empty() ? nullptr : cargs.c_str();
        sh_reads_result r{};
        sh_status st = sh_kraken_run(&k, &r);
        if (st != SH_OK) { fprintf(stderr, "error (%d): %s\n", st, sh_last_error()); return 1; }
        fprintf(stderr, "[scrubby-hip] depleted ids: %llu | database %.0f ms, ingest %.0f ms, classify %.0f ms, write %.0f ms\n",
                (unsigned long long)r.n_depleted_ids, r.ms_index, r.ms_ingest, r.ms_classify, r.ms_write);
        return 0;
    }
    if (aligner.empty()) aligner = "minimap2-rs";
    if (aligner != "minimap2-rs") { fprintf(stderr, "error: the HIP backend replaces --aligner minimap2-rs only (got %s)\n", aligner.c_str()); return 2; }
    if (index.empty()) { fprintf(stderr, "error: MissingAlignmentIndex (-I)\n"); return 2; }
    sh_reads_config c{};
    for (size_t k = 0; k < in.size(); ++k) { c.input[k] = in[k].c_str(); c.output[k] = out[k].c_str(); }
    c.n_files = (uint32_t)in.size(); c.extract = extract; c.index = index.c_str();
    c.preset = preset.empty() ? nullptr : preset.c_str();
    c.json = json.empty() ? nullptr : json.c_str(); c.read_ids = ids.empty() ? nullptr : ids.c_str();
    c.command = command.c_str(); c.threads = threads; c.device = 0;
    sh_reads_result r{};
    sh_status st = sh_reads_run(&c, &r);
    if (st != SH_OK) { fprintf(stderr, "error (%d): %s\n", st, sh_last_error()); return 1; }
    fprintf(stderr, "[scrubby-hip] depleted ids: %llu | index %.0f ms, ingest %.0f ms, classify %.0f ms, write %.0f ms\n",
            (unsigned long long)r.n_depleted_ids, r.ms_index, r.ms_ingest, r.ms_classify, r.ms_write);
    return 0;
}
