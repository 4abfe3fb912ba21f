"""Plain-Python model of the abundance re-estimation (DESIGN.md §7 "Abundance re-estimation"), written from the definitions in
include/scrubby_hip.h, not from the kernels or the host code: the window distribution over per-k-mer codes, the kmer_distrib
file, Bracken's estimate and its table.  Shared by tests/test_k2_bracken_cpu.py, tests/test_k2_bracken_gpu.py and
tests/golden/make_k2_bracken.py."""
import math

AMBIGUOUS = 0xFFFFFFFF
HEADER = "mapped_taxid\tgenome_taxids:kmers_mapped:total_genome_kmers"
LEVEL_RANK = {"D": "superkingdom", "K": "kingdom", "P": "phylum", "C": "class", "O": "order", "F": "family", "G": "genus", "S": "species"}


def window_calls(codes, W, resolve):
    """the call of every window of W consecutive k-mers; resolve(taxa, counts) is ResolveTree over a non-empty multiset"""
    n = len(codes) - W + 1
    if n <= 0:
        return []
    counts, cache, calls = {}, {}, []

    def call():
        if not counts:
            return 0
        key = frozenset(counts.items())
        if key not in cache:
            t = sorted(counts)
            cache[key] = int(resolve(t, [counts[x] for x in t]))
        return cache[key]

    def counted(c):
        return c != 0 and c != AMBIGUOUS

    for c in codes[:W]:
        c = int(c)
        if counted(c):
            counts[c] = counts.get(c, 0) + 1
    cur = call()
    calls.append(cur)
    for p in range(1, n):
        out, inn = int(codes[p - 1]), int(codes[p + W - 1])
        if out != inn:
            if counted(out):
                counts[out] -= 1
                if not counts[out]:
                    del counts[out]
            if counted(inn):
                counts[inn] = counts.get(inn, 0) + 1
            cur = call()
        calls.append(cur)
    return calls


def distribution(record_codes, taxa, n_nodes, k, read_len, resolve):
    """(entries, totals): entries {(genome, call): windows} with call 0 included, totals {genome: windows}; record_codes[i] holds one
    code per k-mer of record i (len - k + 1 of them, none for a shorter record)"""
    W = read_len - k + 1
    entries, totals = {}, {}
    for codes, g in zip(record_codes, taxa):
        g = int(g)
        if g == 0 or g >= n_nodes:
            continue
        for c in window_calls(codes, W, resolve):
            entries[(g, c)] = entries.get((g, c), 0) + 1
            totals[g] = totals.get(g, 0) + 1
    return entries, totals


def distrib_text(entries, totals, external):
    """the kmer_distrib file: one line per mapped taxon (external ids ascending), genomes ascending, call 0 left out"""
    rows = {}
    for (g, m), n in entries.items():
        if m == 0 or n == 0:
            continue
        rows.setdefault(int(external[m]), []).append((int(external[g]), n, totals[g]))
    out = [HEADER]
    for m in sorted(rows):
        out.append(f"{m}\t" + " ".join(f"{g}:{n}:{t}" for g, n, t in sorted(rows[m])))
    return "\n".join(out) + "\n"


def parse_distrib(text, external):
    """(entries, totals) of a kmer_distrib file by internal id; taxids outside `external` are skipped"""
    e2i = {int(x): i for i, x in enumerate(external) if i}
    lines = text.split("\n")
    assert lines[0] == HEADER and lines[-1] == ""
    entries, totals = {}, {}
    for ln in lines[1:-1]:
        m, rest = ln.split("\t")
        for item in rest.split(" "):
            g, n, t = (int(x) for x in item.split(":"))
            if g not in e2i:
                continue
            totals[e2i[g]] = t
            if int(m) in e2i:
                entries[(e2i[g], e2i[int(m)])] = n
    return entries, totals


def parse_report(text, external):
    """direct reads by internal id from a Kraken-style report (rows matched by the taxid column), and the reads of taxids that
    `external` lacks"""
    e2i = {int(x): i for i, x in enumerate(external) if i}
    direct, lost = [0] * len(external), 0
    for ln in text.splitlines():
        f = ln.split("\t")
        taxid, n = int(f[4]), int(f[2])
        if taxid == 0:
            direct[0] += n
        elif taxid in e2i:
            direct[e2i[taxid]] += n
        else:
            lost += n
    return direct, lost


def estimate(parent, ranks, external, names, direct, entries, totals, level="S", threshold=10):
    """Bracken's estimate by the rule of include/scrubby_hip.h.  parent / ranks / external / names / direct: per internal id;
    entries {(genome, mapped): windows}; totals {genome: windows}.  Returns a dict: rows [(taxon, assigned, added, new_est,
    fraction)] by ascending internal id, the summary counts, and `text`, the table sh_k2_bracken_write writes."""
    n = len(parent)
    rank = LEVEL_RANK[level]
    lvl = [0] * n
    for i in range(1, n):
        lvl[i] = i if ranks[i] == rank else (0 if i == 1 else lvl[parent[i]])
    clade = [int(x) for x in direct]
    clade[0] = 0
    for i in range(n - 1, 1, -1):
        clade[parent[i]] += clade[i]
    floor_reads = max(int(threshold), 1)
    kept = [i for i in range(1, n) if lvl[i] == i and clade[i] >= floor_reads]
    below = sum(clade[i] for i in range(1, n) if lvl[i] == i and clade[i] < floor_reads)
    T = {s: sum(int(totals.get(g, 0)) for g in range(1, n) if lvl[g] == s) for s in kept}
    added = {s: 0.0 for s in kept}
    distributed = undistributed = 0
    for x in range(1, n):
        if int(direct[x]) == 0 or lvl[x] != 0:
            continue
        w, total = [], 0.0
        for s in kept:
            m = sum(int(entries.get((g, x), 0)) for g in range(1, n) if lvl[g] == s)
            ws = float(m) / float(T[s]) * float(clade[s]) if T[s] else 0.0
            w.append((s, ws))
            total += ws
        if not total > 0.0:
            undistributed += int(direct[x])
            continue
        distributed += int(direct[x])
        for s, ws in w:
            added[s] += float(int(direct[x])) * ws / total
    new_est = {s: int(math.floor(float(clade[s]) + added[s] + 0.5)) for s in kept}
    whole = sum(new_est.values())
    rows = [(s, clade[s], added[s], new_est[s], (new_est[s] / whole if whole else 0.0)) for s in kept]
    lines = ["name\ttaxonomy_id\ttaxonomy_lvl\tkraken_assigned_reads\tadded_reads\tnew_est_reads\tfraction_total_reads"]
    for s, a, _, e, f in sorted(rows, key=lambda r: int(external[r[0]])):
        lines.append(f"{names[s]}\t{int(external[s])}\t{level}\t{a}\t{e - a}\t{e}\t{f:.5f}")
    return {"rows": rows, "reads_total": sum(int(x) for x in direct[1:]), "reads_at_level": sum(clade[s] for s in kept), "reads_below_threshold": below,
            "reads_distributed": distributed, "reads_undistributed": undistributed, "new_est_total": whole, "text": "\n".join(lines) + "\n"}
