"""ctypes binding of the Kraken2-style taxid path of libscrubby_hip.so (include/scrubby_hip.h, `sh_k2_*`, `sh_kraken_run`).

Mirrors what the reference reaches through the external `kraken2` process (Cleaner::run_kraken,
/root/reference/src/cleaner.rs:288-330).  No CPU path: everything here needs the HIP library and a GPU.
"""
import ctypes as C
import os

import numpy as np

from . import lib as S


class K2Opts(C.Structure):
    _fields_ = [("k", C.c_int32), ("l", C.c_int32), ("spaced_seed_mask", C.c_uint64), ("toggle_mask", C.c_uint64),
                ("min_acceptable_hash", C.c_uint64), ("value_bits", C.c_int32), ("min_hit_groups", C.c_int32),
                ("confidence", C.c_double), ("min_base_quality", C.c_int32), ("quick", C.c_int32),
                ("long_unit_bases", C.c_int32), ("protein", C.c_int32)]


class K2TaxNode(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("parent", "first_child", "child_count", "name_offset", "rank_offset", "external_id", "godparent")]


class K2Info(C.Structure):
    _fields_ = [("capacity", C.c_uint64), ("size", C.c_uint64), ("n_nodes", C.c_uint64), ("hbm_bytes", C.c_uint64),
                ("k", C.c_int32), ("l", C.c_int32), ("value_bits", C.c_int32), ("key_bits", C.c_int32)]


class K2Stats(C.Structure):
    _fields_ = [("n_units", C.c_uint64), ("n_classified", C.c_uint64), ("n_probes", C.c_uint64), ("n_kmers", C.c_uint64),
                ("n_overflow", C.c_uint64), ("ms_classify", C.c_float), ("ms_total", C.c_float), ("n_masked_bases", C.c_uint64),
                ("n_long_units", C.c_uint64), ("ms_long", C.c_float), ("ms_translate", C.c_float)]


class KrakenConfig(C.Structure):
    _fields_ = [("input", C.c_char_p * 2), ("output", C.c_char_p * 2), ("n_files", C.c_uint32), ("extract", C.c_int32),
                ("db", C.c_char_p), ("workdir", C.c_char_p),
                ("taxa", C.POINTER(C.c_char_p)), ("n_taxa", C.c_uint32),
                ("taxa_direct", C.POINTER(C.c_char_p)), ("n_taxa_direct", C.c_uint32),
                ("confidence", C.c_double), ("min_hit_groups", C.c_int32),
                ("json", C.c_char_p), ("read_ids", C.c_char_p), ("command", C.c_char_p),
                ("device", C.c_int32), ("threads", C.c_int32), ("classifier_args", C.c_char_p),
                ("min_base_quality", C.c_int32), ("quick", C.c_int32), ("report_minimizer_data", C.c_int32)]


class K2Batch(C.Structure):
    _fields_ = [("bases", C.c_void_p), ("quals", C.c_void_p), ("offsets", C.c_void_p), ("n_records", C.c_uint64), ("paired", C.c_int32)]


class K2TaxonomyInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_uint64), ("names_len", C.c_uint64), ("ranks_len", C.c_uint64), ("value_bits", C.c_int32), ("pad", C.c_int32),
                ("n_map_entries", C.c_uint64), ("n_missing_taxa", C.c_uint64)]


class K2BuildStats(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_segments", C.c_uint64), ("n_runs", C.c_uint64), ("size", C.c_uint64), ("ms", C.c_float)]


class K2BuildConfig(C.Structure):
    _fields_ = [("input", C.POINTER(C.c_char_p)), ("n_input", C.c_uint32), ("taxonomy_dir", C.c_char_p), ("seqid2taxid", C.c_char_p),
                ("taxid", C.c_uint64), ("name", C.c_char_p), ("rank", C.c_char_p), ("output_dir", C.c_char_p),
                ("k", C.c_int32), ("l", C.c_int32), ("minimizer_spaces", C.c_int32), ("value_bits", C.c_int32),
                ("capacity", C.c_uint64), ("load_factor", C.c_double), ("max_db_size", C.c_uint64), ("chunk_bytes", C.c_uint64),
                ("device", C.c_int32), ("pad", C.c_int32),
                ("mask_low_complexity", C.c_int32), ("mask_window", C.c_int32), ("mask_threshold", C.c_int32), ("protein", C.c_int32)]


class K2BuildResult(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_records", "n_skipped", "n_bases", "n_batches", "n_cuts", "n_runs", "size", "capacity", "n_nodes",
                                           "n_sampled", "estimate", "min_acceptable_hash")] + \
               [("value_bits", C.c_int32), ("pad", C.c_int32)] + \
               [(n, C.c_double) for n in ("s_taxonomy", "s_estimate", "s_fill", "s_save", "s_read", "s_total")] + \
               [("n_masked_bases", C.c_uint64), ("s_mask", C.c_double)]


class K2MaskStats(C.Structure):
    _fields_ = [("n_bases", C.c_uint64), ("n_masked", C.c_uint64), ("n_items", C.c_uint64), ("ms", C.c_float), ("pad", C.c_int32)]


class K2MaskConfig(C.Structure):
    _fields_ = [("input", C.c_char_p), ("output", C.c_char_p), ("window", C.c_int32), ("threshold", C.c_int32), ("replacement", C.c_int32),
                ("soft", C.c_int32), ("line_width", C.c_int32), ("device", C.c_int32), ("chunk_bytes", C.c_uint64)]


class K2MaskResult(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_records", "n_bases", "n_masked_bases", "n_batches", "n_cuts")] + \
               [("s_mask", C.c_double), ("s_total", C.c_double)]


class K2InspectStats(C.Structure):
    _fields_ = [("n_cells", C.c_uint64), ("n_occupied", C.c_uint64), ("n_bad_values", C.c_uint64), ("ms", C.c_float), ("pad", C.c_int32)]


class K2InspectConfig(C.Structure):
    _fields_ = [("db", C.c_char_p), ("output", C.c_char_p), ("skip_counts", C.c_int32), ("report_zero_counts", C.c_int32),
                ("use_mpa_style", C.c_int32), ("device", C.c_int32)]


class K2InspectResult(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("capacity", "size_header", "n_occupied", "n_bad_values", "n_nodes", "n_taxa_with_minimizers")] + \
               [(n, C.c_double) for n in ("s_open", "s_count", "s_report", "s_total")]


class K2DistribStats(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_windows", C.c_uint64), ("n_items", C.c_uint64), ("n_big", C.c_uint64), ("ms", C.c_float), ("pad", C.c_int32)]


class K2BrackenRow(C.Structure):
    _fields_ = [("taxon", C.c_uint32), ("pad", C.c_uint32), ("assigned", C.c_uint64), ("new_est", C.c_uint64), ("added", C.c_double), ("fraction", C.c_double)]


class K2BrackenSummary(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_rows", "reads_total", "reads_at_level", "reads_below_threshold", "reads_distributed", "reads_undistributed",
                                           "new_est_total")]


class K2DistribConfig(C.Structure):
    _fields_ = [("db", C.c_char_p), ("input", C.POINTER(C.c_char_p)), ("n_input", C.c_uint32), ("read_len", C.c_int32), ("seqid2taxid", C.c_char_p),
                ("taxid", C.c_uint64), ("output", C.c_char_p), ("chunk_bytes", C.c_uint64), ("device", C.c_int32), ("pad", C.c_int32)]


class K2DistribResult(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_records", "n_skipped", "n_bases", "n_batches", "n_cuts", "n_windows", "n_items", "n_big", "n_entries")] + \
               [(n, C.c_double) for n in ("s_open", "s_gpu", "s_read", "s_write", "s_total")]


class K2BrackenConfig(C.Structure):
    _fields_ = [("db", C.c_char_p), ("report", C.c_char_p), ("read_len", C.c_int32), ("level", C.c_int32), ("threshold", C.c_int64),
                ("kmer_distrib", C.c_char_p), ("output", C.c_char_p)]


class K2BrackenResult(C.Structure):
    _fields_ = [("summary", K2BrackenSummary), ("n_report_rows", C.c_uint64), ("n_unknown_taxa", C.c_uint64)]


INSPECT_ZERO_COUNTS, INSPECT_MPA = 1, 2

RESULT_DTYPE = np.dtype([("taxid", "<u4"), ("call", "<u4"), ("total_kmers", "<u4"), ("hit_groups", "<u4")])
# one hit-list entry: internal taxid (0 = not in the table / not looked up), HIT_AMBIGUOUS or HIT_BORDER, and its k-mer count
HIT_DTYPE = np.dtype([("code", "<u4"), ("count", "<u4")])
HIT_AMBIGUOUS, HIT_BORDER = 0xFFFFFFFF, 0xFFFFFFFE


def format_hits(entries, external, quick=False, quick_taxid=0):
    """Column 5 of kraken.reads for one unit (sh_k2_format_hits; host only, no GPU needed): entries = HIT_DTYPE array or
    (code, count) pairs, external = the taxonomy's external ids by internal id."""
    e = np.ascontiguousarray(np.array([tuple(x) for x in entries], dtype=HIT_DTYPE) if not isinstance(entries, np.ndarray) else entries, dtype=HIT_DTYPE)
    ext = np.ascontiguousarray(external, dtype=np.uint32)
    n = C.c_uint64()
    L = S.load()
    args = (C.c_void_p(e.ctypes.data), C.c_uint64(len(e)), C.c_void_p(ext.ctypes.data), C.c_uint64(len(ext)), int(bool(quick)), C.c_uint32(quick_taxid))
    S.check(L.sh_k2_format_hits(*args, None, C.c_uint64(0), C.byref(n)))
    buf = C.create_string_buffer(n.value + 1)
    S.check(L.sh_k2_format_hits(*args, buf, C.c_uint64(n.value + 1), C.byref(n)))
    return buf.value.decode()


# one entry of a k-mer distribution: of the windows of library genome `genome`, `windows` are called `mapped` (internal ids; 0 = unclassified)
DISTRIB_DTYPE = np.dtype([("genome", "<u4"), ("mapped", "<u4"), ("windows", "<u8")])
BRACKEN_ROW_DTYPE = np.dtype([("taxon", "<u4"), ("pad", "<u4"), ("assigned", "<u8"), ("new_est", "<u8"), ("added", "<f8"), ("fraction", "<f8")])


# k-mers per tile of the wave route (sh_k2_wave_tile; units of at least opts.long_unit_bases bases are classified one wave each)
K2_WAVE_TILE = 64 * 63


def _stats_dict(st):
    return {n: getattr(st, n) for n, _ in K2Stats._fields_}


def _take_hits(h):
    """offsets (n_units + 1) and entries of a sh_k2_hits handle copied to the host, and the units its overflow pass redid;
    the handle is freed"""
    L = S.load()
    try:
        nu, ne, nr = C.c_uint64(), C.c_uint64(), C.c_uint64()
        S.check(L.sh_k2_hits_count(h, C.byref(nu), C.byref(ne), C.byref(nr)))
        offs = np.zeros(nu.value + 1, dtype=np.uint64)
        ent = np.zeros(max(ne.value, 1), dtype=HIT_DTYPE)
        S.check(L.sh_k2_hits_copy(h, C.c_void_p(offs.ctypes.data), C.c_void_p(ent.ctypes.data)))
        return offs, ent[: ne.value], nr.value
    finally:
        L.sh_k2_hits_free(h)


HLL_REGISTERS = 4096        # per taxon, one byte each (precision 12)


def hll_estimate(regs):
    """Distinct-count estimate of 4096 HyperLogLog registers (sh_k2_hll_estimate: Ertl's improved raw estimator; host only)"""
    r = np.ascontiguousarray(regs, dtype=np.uint8)
    assert r.shape == (HLL_REGISTERS,), "4096 registers"
    e = C.c_double()
    S.check(S.load().sh_k2_hll_estimate(C.c_void_p(r.ctypes.data), C.byref(e)))
    return e.value


def hll_merge(dst, src):
    """element-wise maximum of two register arrays into dst (sh_k2_mindata_merge_host; host only)"""
    assert dst.dtype == np.uint8 and dst.flags.c_contiguous and dst.flags.writeable and len(dst) == len(src)
    s = np.ascontiguousarray(src, dtype=np.uint8)
    S.check(S.load().sh_k2_mindata_merge_host(C.c_void_p(dst.ctypes.data), C.c_void_p(s.ctypes.data), C.c_uint64(len(dst))))
    return dst


def write_minimizer_report(nodes, names, ranks, clade_reads, direct_reads, clade_minimizers, clade_distinct, total_units, path):
    """kraken2 --report-minimizer-data's 8-column report (sh_k2_write_minimizer_report; host only) over a taxonomy in taxo.k2d's
    layout and four per-taxon arrays"""
    a = [np.ascontiguousarray(x, dtype=np.uint64) for x in (clade_reads, direct_reads, clade_minimizers, clade_distinct)]
    assert all(len(x) == len(nodes) for x in a), "one value per taxonomy node"
    S.check(S.load().sh_k2_write_minimizer_report(nodes, C.c_uint64(len(nodes)), names, C.c_uint64(len(names)), ranks, C.c_uint64(len(ranks)),
                                                  *[C.c_void_p(x.ctypes.data) for x in a], C.c_uint64(total_units), str(path).encode()))


class MinimizerData:
    """The per-taxon minimizer counts and HyperLogLog registers of one database (sh_k2_mindata), kept in HBM; classify calls
    given `minimizer_data=` add to it."""

    def __init__(self, db):
        self.n_nodes = db.info()["n_nodes"]
        self.h = C.c_void_p()
        S.check(S.load().sh_k2_mindata_create(db.h, C.byref(self.h)))

    def reset(self):
        S.check(S.load().sh_k2_mindata_reset(self.h))

    def counts(self):
        """dict of four arrays by internal taxon: n_minimizers, clade_minimizers (uint64), distinct, clade_distinct (float64)"""
        n = self.n_nodes
        r = {"n_minimizers": np.zeros(n, np.uint64), "clade_minimizers": np.zeros(n, np.uint64), "distinct": np.zeros(n, np.float64),
             "clade_distinct": np.zeros(n, np.float64)}
        S.check(S.load().sh_k2_mindata_counts(self.h, *[C.c_void_p(r[k].ctypes.data) for k in ("n_minimizers", "clade_minimizers", "distinct", "clade_distinct")]))
        return r

    def registers(self, taxon, clade=False):
        out = np.zeros(HLL_REGISTERS, dtype=np.uint8)
        S.check(S.load().sh_k2_mindata_registers(self.h, C.c_uint32(taxon), C.c_void_p(out.ctypes.data), int(bool(clade))))
        return out

    def close(self):
        if self.h:
            S.load().sh_k2_mindata_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_opts():
    o = K2Opts()
    S.check(S.load().sh_k2_default_opts(C.byref(o)))
    return o


def default_protein_opts():
    """the defaults of a protein database (sh_k2_default_protein_opts): k 15, l 12 amino acids, no spaced seed, protein = 1"""
    o = K2Opts()
    S.check(S.load().sh_k2_default_protein_opts(C.byref(o)))
    return o


AA_AMBIGUOUS = 0x80         # a translated code byte that is no amino acid of the reduced alphabet (X)


def _records_flat(records, pad, fill):
    arrs = [np.frombuffer(bytes(r), dtype=np.uint8) if not isinstance(r, np.ndarray) else np.ascontiguousarray(r, dtype=np.uint8) for r in records]
    off = np.zeros(len(arrs) + 1, dtype=np.uint64)
    if arrs:
        off[1:] = np.cumsum([len(a) for a in arrs], dtype=np.uint64)
    return np.concatenate(arrs + [np.full(pad, fill, np.uint8)]), off


def translate_host(records, quals=None, min_qual=0, as_letters=False):
    """Six-frame translation on the CPU (sh_k2_translate_host; no GPU needed) of a list of nucleotide sequences (quals: a list of
    Phred+33 byte strings, or None).  Returns (out, offsets): record r's frames 0..5 lie back to back from
    out[2 * offsets[r]], (n-1)//3, (n-2)//3 and n//3 residues forward and as many reverse; scanner codes 0..15 and AA_AMBIGUOUS,
    or with as_letters the residues themselves.  Bytes between records are zero."""
    flat, off = _records_flat(records, 8, ord("N"))
    q = _records_flat(quals, 8, 0xff)[0] if quals is not None else None
    out = np.zeros(2 * int(off[-1]) + 8, dtype=np.uint8)
    S.check(S.load().sh_k2_translate_host(C.c_void_p(flat.ctypes.data), C.c_void_p(q.ctypes.data) if q is not None else None, C.c_void_p(off.ctypes.data),
                                          C.c_uint64(len(off) - 1), C.c_int32(min_qual), C.c_int32(int(bool(as_letters))), C.c_void_p(out.ctypes.data)))
    return out, off


def translate_device(records, quals=None, min_qual=0, as_letters=False, misalign=0):
    """The same on the GPU (sh_k2_translate_device, k_k2_translate).  misalign: the batch's first base sits that many bytes behind
    an 8-byte boundary (and offsets[0] = misalign), the output starts as many bytes behind one."""
    import torch
    S.require_gpu()
    flat, off = _records_flat([b"N" * misalign] + list(records) if misalign else records, 8, ord("N"))
    n_rec = len(off) - 1 - (1 if misalign else 0)
    d_bases = torch.from_numpy(flat).cuda()
    d_off = torch.from_numpy(off[1 if misalign else 0:].view(np.int64).copy()).cuda()
    d_q = None
    if quals is not None:
        d_q = torch.from_numpy(_records_flat([b"!" * misalign] + list(quals) if misalign else quals, 8, 0xff)[0]).cuda()
    n_bases = int(off[-1]) - misalign
    d_out = torch.zeros(2 * n_bases + 8 + misalign, dtype=torch.uint8, device="cuda")
    S.check(S.load().sh_k2_translate_device(C.c_void_p(d_bases.data_ptr()), C.c_void_p(d_q.data_ptr()) if d_q is not None else None, C.c_void_p(d_off.data_ptr()),
                                            C.c_uint64(n_rec), C.c_int32(min_qual), C.c_int32(int(bool(as_letters))), C.c_void_p(d_out.data_ptr() + misalign),
                                            S._stream_ptr()))
    torch.cuda.synchronize()
    return d_out.cpu().numpy()[misalign:], (off[1 if misalign else 0:] - np.uint64(misalign))


def make_taxonomy(parents, externals, names, ranks):
    """Node arrays for sh_k2_create from per-node lists (index = internal id; entry 0 is the unused sentinel)."""
    n = len(parents)
    nodes = (K2TaxNode * n)()
    name_pool, rank_pool = bytearray(), bytearray()
    kids = [[] for _ in range(n)]
    for i in range(2, n):
        assert parents[i] < i, "ids must be breadth-first"
        kids[parents[i]].append(i)
    for i in range(n):
        nodes[i].parent = parents[i]
        nodes[i].external_id = externals[i]
        nodes[i].name_offset = len(name_pool); name_pool += names[i].encode() + b"\0"
        nodes[i].rank_offset = len(rank_pool); rank_pool += ranks[i].encode() + b"\0"
        if kids[i]:
            assert kids[i] == list(range(kids[i][0], kids[i][0] + len(kids[i]))), "children must have consecutive ids"
            nodes[i].first_child, nodes[i].child_count = kids[i][0], len(kids[i])
    return nodes, bytes(name_pool), bytes(rank_pool)


class Taxonomy:
    """An NCBI taxonomy reduced to the taxa a library uses, in taxo.k2d's layout (sh_k2_taxonomy_*; host only, no GPU needed)."""

    def __init__(self, handle):
        self.h = handle

    def info(self):
        i = K2TaxonomyInfo()
        S.check(S.load().sh_k2_taxonomy_info_get(self.h, C.byref(i)))
        return {n: getattr(i, n) for n, _ in K2TaxonomyInfo._fields_ if n != "pad"}

    def arrays(self):
        """(nodes, names, ranks): a K2TaxNode array and the two string pools"""
        i = self.info()
        nodes = (K2TaxNode * i["n_nodes"])()
        names, ranks = C.create_string_buffer(max(i["names_len"], 1)), C.create_string_buffer(max(i["ranks_len"], 1))
        S.check(S.load().sh_k2_taxonomy_copy(self.h, nodes, names, ranks))
        return nodes, names.raw[: i["names_len"]], ranks.raw[: i["ranks_len"]]

    def internal(self, external_id):
        r = C.c_uint32()
        S.check(S.load().sh_k2_taxonomy_internal(self.h, C.c_uint64(external_id), C.byref(r)))
        return r.value

    def header_taxon(self, header):
        """internal taxon of the record with this FASTA header (without '>'); 0 = the record is skipped"""
        hb = header if isinstance(header, bytes) else header.encode()
        r = C.c_uint32()
        S.check(S.load().sh_k2_taxonomy_header_taxon(self.h, hb, C.c_uint64(len(hb)), C.byref(r)))
        return r.value

    def close(self):
        if self.h:
            S.load().sh_k2_taxonomy_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def taxonomy_from_ncbi(nodes_dmp, names_dmp, seqid2taxid=None, extra_taxids=(), value_bits=0):
    ex = (C.c_uint64 * max(len(extra_taxids), 1))(*extra_taxids)
    h = C.c_void_p()
    S.check(S.load().sh_k2_taxonomy_from_ncbi(str(nodes_dmp).encode(), str(names_dmp).encode(), str(seqid2taxid).encode() if seqid2taxid else None,
                                              ex, C.c_uint64(len(extra_taxids)), value_bits, C.byref(h)))
    return Taxonomy(h)


def taxonomy_single(taxid, name=None, rank=None, value_bits=0):
    h = C.c_void_p()
    S.check(S.load().sh_k2_taxonomy_single(C.c_uint64(taxid), name.encode() if name else None, rank.encode() if rank else None, value_bits, C.byref(h)))
    return Taxonomy(h)


def capacity_plan(n_sampled, load_factor=0.7, max_db_size=0):
    """(estimate, capacity, min_acceptable_hash) from the estimator's distinct sample count"""
    e, c, m = C.c_uint64(), C.c_uint64(), C.c_uint64()
    S.check(S.load().sh_k2_capacity_plan(C.c_uint64(n_sampled), C.c_double(load_factor), C.c_uint64(max_db_size), C.byref(e), C.byref(c), C.byref(m)))
    return e.value, c.value, m.value


def max_db_size(needed_capacity, max_bytes):
    """kraken2-build --max-db-size on a known capacity: (capacity, min_acceptable_hash)"""
    c, m = C.c_uint64(), C.c_uint64()
    S.check(S.load().sh_k2_max_db_size(C.c_uint64(needed_capacity), C.c_uint64(max_bytes), C.byref(c), C.byref(m)))
    return c.value, m.value


def _library_to_device(records):
    """records: byte strings / uint8 arrays -> (d_bases with 64 bytes of padding, d_offsets, n_records) as torch tensors"""
    import torch
    arrs = [np.frombuffer(bytes(r), dtype=np.uint8) if not isinstance(r, np.ndarray) else r for r in records]
    off = np.zeros(len(arrs) + 1, dtype=np.uint64)
    if arrs:
        off[1:] = np.cumsum([len(a) for a in arrs], dtype=np.uint64)
    flat = np.concatenate(arrs + [np.full(64, ord("N"), np.uint8)])
    return torch.from_numpy(flat).cuda(), torch.from_numpy(off.view(np.int64)).cuda(), len(arrs)


def estimate_capacity(records, opts=None, batches=1, load_factor=0.7, max_db_size=0, device=0):
    """Kraken 2's capacity estimate of a library given as a list of sequences, fed to one estimator in `batches` calls:
    dict with n_sampled, estimate, capacity, min_acceptable_hash."""
    S.require_gpu()
    L = S.load()
    o = opts if opts is not None else default_opts()
    h = C.c_void_p()
    S.check(L.sh_k2_estimator_create(C.byref(o), device, C.byref(h)))
    try:
        n = C.c_uint64()
        step = max((len(records) + batches - 1) // batches, 1)
        for b in range(0, len(records), step):
            d_bases, d_off, nr = _library_to_device(records[b: b + step])
            S.check(L.sh_k2_estimate_capacity_device(h, C.c_void_p(d_bases.data_ptr()), C.c_void_p(d_off.data_ptr()), C.c_uint64(nr), None, C.byref(n)))
    finally:
        L.sh_k2_estimator_free(h)
    est, cap, mh = capacity_plan(n.value, load_factor, max_db_size)
    return {"n_sampled": n.value, "estimate": est, "capacity": cap, "min_acceptable_hash": mh}


def _replacement_code(replacement):
    """b"x" / "x" / 120 -> 120; None, b"" or 0 -> 0 (soft masking: lower case)"""
    if not replacement:
        return 0
    if isinstance(replacement, int):
        return replacement
    r = replacement if isinstance(replacement, bytes) else str(replacement).encode()
    assert len(r) == 1, "the replacement is one byte"
    return r[0]


def _mask_stats(st):
    return {n: getattr(st, n) for n, _ in K2MaskStats._fields_ if n != "pad"}


def _inspect_stats(st):
    return {n: getattr(st, n) for n, _ in K2InspectStats._fields_ if n != "pad"}


def mask_low_complexity(records, window=64, threshold=20, replacement=b"x", return_stats=False):
    """Symmetric DUST on the GPU (sh_k2_mask_device) over a list of sequences; replacement None / 0 = soft masking (lower case).
    Returns the masked sequences as bytes, in order (and the call's statistics with return_stats=True)."""
    S.require_gpu()
    d_bases, d_off, n = _library_to_device(records)
    st = K2MaskStats()
    S.check(S.load().sh_k2_mask_device(C.c_void_p(d_bases.data_ptr()), C.c_void_p(d_off.data_ptr()), C.c_uint64(n), window, threshold,
                                       _replacement_code(replacement), S._stream_ptr(), C.byref(st)))
    flat = d_bases.cpu().numpy()
    off = d_off.cpu().numpy()
    out = [flat[int(off[i]): int(off[i + 1])].tobytes() for i in range(n)]
    return (out, _mask_stats(st)) if return_stats else out


def mask_low_complexity_host(records, window=64, threshold=20, replacement=b"x", return_stats=False):
    """The same on the CPU (sh_k2_mask_host, the streaming mirror; no GPU needed)."""
    arrs = [np.frombuffer(bytes(r), dtype=np.uint8) for r in records]
    off = np.zeros(len(arrs) + 1, dtype=np.uint64)
    if arrs:
        off[1:] = np.cumsum([len(a) for a in arrs], dtype=np.uint64)
    flat = np.concatenate(arrs + [np.zeros(8, np.uint8)]).copy()
    st = K2MaskStats()
    S.check(S.load().sh_k2_mask_host(C.c_void_p(flat.ctypes.data), C.c_void_p(off.ctypes.data), C.c_uint64(len(arrs)), window, threshold,
                                     _replacement_code(replacement), C.byref(st)))
    out = [flat[int(off[i]): int(off[i + 1])].tobytes() for i in range(len(arrs))]
    return (out, _mask_stats(st)) if return_stats else out


def mask_file(input, output, window=0, threshold=0, replacement=b"x", soft=False, line_width=60, chunk_bytes=0, device=0):
    """`scrubby-hip k2-mask` (sh_k2_mask_run): FASTA in, masked FASTA out; returns the result fields as a dict."""
    S.require_gpu()
    c = K2MaskConfig()
    c.input, c.output = str(input).encode(), str(output).encode()
    c.window, c.threshold, c.replacement, c.soft = window, threshold, _replacement_code(replacement), int(bool(soft))
    c.line_width, c.device, c.chunk_bytes = line_width, device, chunk_bytes
    r = K2MaskResult()
    S.check(S.load().sh_k2_mask_run(C.byref(c), C.byref(r)))
    return {n: getattr(r, n) for n, _ in K2MaskResult._fields_}


def build_database(inputs, output_dir, taxonomy_dir=None, seqid2taxid=None, taxid=0, name=None, rank=None, k=0, l=0, minimizer_spaces=0,
                   capacity=0, load_factor=0.0, max_db_size=0, value_bits=0, chunk_bytes=0, device=0, mask=False, mask_window=0,
                   mask_threshold=0, protein=False):
    """`scrubby-hip k2-build` (sh_k2_build_run): FASTA library files + (taxonomy directory [+ id map] | one taxid) -> a database
    directory.  minimizer_spaces: 0 = Kraken 2's 7, negative = none.  mask=True: low-complexity sequence is masked on the GPU
    before both passes (kraken2-build's default; off here).  protein=True: kraken2-build --protein, an amino-acid FASTA library
    (defaults k 15, l 12, no minimizer spaces; mask=True is then refused).  Returns the result fields as a dict."""
    S.require_gpu()
    c = K2BuildConfig()
    files = [inputs] if isinstance(inputs, (str, bytes)) or hasattr(inputs, "__fspath__") else list(inputs)
    arr = (C.c_char_p * len(files))(*[str(f).encode() for f in files])
    c.input, c.n_input = arr, len(files)
    c.taxonomy_dir = str(taxonomy_dir).encode() if taxonomy_dir else None
    c.seqid2taxid = str(seqid2taxid).encode() if seqid2taxid else None
    c.taxid, c.name, c.rank = taxid, name.encode() if name else None, rank.encode() if rank else None
    c.output_dir = str(output_dir).encode()
    c.k, c.l, c.minimizer_spaces, c.value_bits = k, l, minimizer_spaces, value_bits
    c.capacity, c.load_factor, c.max_db_size, c.chunk_bytes, c.device = capacity, load_factor, max_db_size, chunk_bytes, device
    c.mask_low_complexity, c.mask_window, c.mask_threshold = int(bool(mask)), mask_window, mask_threshold
    c.protein = int(bool(protein))
    r = K2BuildResult()
    S.check(S.load().sh_k2_build_run(C.byref(c), C.byref(r)))
    return {n: getattr(r, n) for n, _ in K2BuildResult._fields_ if n != "pad"}


def counts_report(nodes, names, ranks, counts, path, zero_counts=False, mpa=False, header=None):
    """kraken2-inspect's report (sh_k2_counts_report; host only, no GPU needed) over a taxonomy in taxo.k2d's layout (a K2TaxNode
    array and the two string pools, as Taxonomy.arrays() gives them) and one count per node; header (optional) is written first,
    verbatim; path None or "-" = stdout."""
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    assert len(c) == len(nodes), "one count per taxonomy node"
    flags = (INSPECT_ZERO_COUNTS if zero_counts else 0) | (INSPECT_MPA if mpa else 0)
    hb = None if header is None else (header if isinstance(header, bytes) else header.encode())
    S.check(S.load().sh_k2_counts_report(nodes, C.c_uint64(len(nodes)), names, C.c_uint64(len(names)), ranks, C.c_uint64(len(ranks)),
                                         C.c_void_p(c.ctypes.data), flags, hb, None if path is None else str(path).encode()))


def inspect_database(db_dir, output=None, skip_counts=False, report_zero_counts=False, use_mpa_style=False, device=0):
    """`scrubby-hip k2-inspect` (sh_k2_inspect_run): the header lines and the per-taxon minimizer report of a database directory,
    to `output` or stdout; returns the result fields as a dict."""
    S.require_gpu()
    c = K2InspectConfig()
    c.db, c.output = str(db_dir).encode(), str(output).encode() if output else None
    c.skip_counts, c.report_zero_counts, c.use_mpa_style, c.device = int(bool(skip_counts)), int(bool(report_zero_counts)), int(bool(use_mpa_style)), device
    r = K2InspectResult()
    S.check(S.load().sh_k2_inspect_run(C.byref(c), C.byref(r)))
    return {n: getattr(r, n) for n, _ in K2InspectResult._fields_}


def distrib_stretch():
    """window starts per work item of the window kernel (sh_k2_distrib_stretch)"""
    return int(S.load().sh_k2_distrib_stretch())


class KmerDistrib:
    """bracken-build's k-mer distribution of one database at one read length (sh_k2_distrib), accumulated in HBM: for every
    window of read_len bases of every library record, what Kraken 2 would call it.  Calls add up in any batching."""

    def __init__(self, db, read_len):
        S.require_gpu()
        self.db, self.read_len = db, read_len          # the database must outlive the accumulator
        self.n_nodes = db.info()["n_nodes"]
        self.h = C.c_void_p()
        S.check(S.load().sh_k2_distrib_create(db.h, C.c_int32(read_len), C.byref(self.h)))

    def add_device(self, d_bases, d_offsets, d_taxa, n_records):
        """sh_k2_distrib_add_device on torch tensors (uint8 bases readable 8 bytes past the end, int64 offsets, int32 taxa);
        returns the call's statistics"""
        st = K2DistribStats()
        S.check(S.load().sh_k2_distrib_add_device(self.h, C.c_void_p(d_bases.data_ptr()), C.c_void_p(d_offsets.data_ptr()), C.c_void_p(d_taxa.data_ptr()),
                                                  C.c_uint64(n_records), S._stream_ptr(), C.byref(st)))
        return {n: getattr(st, n) for n, _ in K2DistribStats._fields_ if n != "pad"}

    def add_library(self, records, taxa, misalign=0):
        """One call over a list of sequences, record i under internal taxon taxa[i] (0 = skip).  misalign: the batch's first base
        sits that many bytes behind an 8-byte boundary."""
        import torch
        assert len(records) == len(taxa)
        d_bases, d_off, n = _library_to_device([b"N" * misalign] + list(records) if misalign else records)
        t = ([0] if misalign else []) + [int(x) for x in taxa]
        d_taxa = torch.from_numpy(np.asarray(t + [0], dtype=np.uint32).view(np.int32).copy()).cuda()
        return self.add_device(d_bases, d_off, d_taxa, n)

    def last_ms(self):
        """(codes kernel, window kernels) milliseconds of the last call"""
        a, b = C.c_float(), C.c_float()
        S.check(S.load().sh_k2_distrib_last_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def _copy(self):
        n = C.c_uint64()
        S.check(S.load().sh_k2_distrib_count(self.h, C.byref(n)))
        ent = np.zeros(max(n.value, 1), dtype=DISTRIB_DTYPE)
        tot = np.zeros(self.n_nodes, dtype=np.uint64)
        S.check(S.load().sh_k2_distrib_copy(self.h, C.c_void_p(ent.ctypes.data), C.c_void_p(tot.ctypes.data)))
        return ent[: n.value], tot

    def entries(self):
        """DISTRIB_DTYPE array sorted by (genome, mapped), unclassified windows (mapped 0) included"""
        return self._copy()[0]

    def totals(self):
        """windows per genome (uint64 by internal id), unclassified ones included"""
        return self._copy()[1]

    def reset(self):
        S.check(S.load().sh_k2_distrib_reset(self.h))

    def close(self):
        if self.h:
            S.load().sh_k2_distrib_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_kmer_distrib(entries, totals, external, read_len, path):
    """Bracken's database<L>mers.kmer_distrib (sh_k2_distrib_write; host only, no GPU needed): entries = DISTRIB_DTYPE array,
    totals = windows per genome, external = the taxonomy's external ids, both by internal id"""
    e = np.ascontiguousarray(entries, dtype=DISTRIB_DTYPE)
    t = np.ascontiguousarray(totals, dtype=np.uint64)
    x = np.ascontiguousarray(external, dtype=np.uint32)
    assert len(t) == len(x), "one total per taxonomy node"
    S.check(S.load().sh_k2_distrib_write(C.c_void_p(e.ctypes.data), C.c_uint64(len(e)), C.c_void_p(t.ctypes.data), C.c_void_p(x.ctypes.data), C.c_uint64(len(x)),
                                         C.c_int32(read_len), str(path).encode()))


def read_kmer_distrib(path, external):
    """(entries, totals) of a kmer_distrib file (sh_k2_distrib_read; host only): entries sorted by (genome, mapped), internal ids"""
    x = np.ascontiguousarray(external, dtype=np.uint32)
    n = C.c_uint64()
    head = (str(path).encode(), C.c_void_p(x.ctypes.data), C.c_uint64(len(x)))
    tot = np.zeros(len(x), dtype=np.uint64)
    # room for every (genome, mapped) pair the file can hold is not known before it is read: size from its bytes (an entry has 5 at least)
    cap = os.path.getsize(path) // 5 + 1
    ent = np.zeros(cap, dtype=DISTRIB_DTYPE)
    S.check(S.load().sh_k2_distrib_read(*head, C.c_void_p(ent.ctypes.data), C.c_uint64(cap), C.byref(n), C.c_void_p(tot.ctypes.data)))
    return ent[: n.value].copy(), tot


def bracken_estimate(nodes, ranks, direct_reads, entries, totals, level="S", threshold=10):
    """Bracken's estimate (sh_k2_bracken_estimate; host only) over a taxonomy in taxo.k2d's layout: (rows, summary) with rows a
    BRACKEN_ROW_DTYPE array by ascending internal id of the kept taxa and summary a dict"""
    d = np.ascontiguousarray(direct_reads, dtype=np.uint64)
    e = np.ascontiguousarray(entries, dtype=DISTRIB_DTYPE)
    t = np.ascontiguousarray(totals, dtype=np.uint64)
    assert len(d) == len(nodes) and len(t) == len(nodes), "one value per taxonomy node"
    rows = np.zeros(len(nodes), dtype=BRACKEN_ROW_DTYPE)
    sm = K2BrackenSummary()
    S.check(S.load().sh_k2_bracken_estimate(nodes, C.c_uint64(len(nodes)), ranks, C.c_uint64(len(ranks)), C.c_void_p(d.ctypes.data), C.c_void_p(e.ctypes.data),
                                            C.c_uint64(len(e)), C.c_void_p(t.ctypes.data), C.c_int32(ord(level)), C.c_uint64(threshold),
                                            C.c_void_p(rows.ctypes.data), C.byref(sm)))
    return rows[: sm.n_rows].copy(), {n: getattr(sm, n) for n, _ in K2BrackenSummary._fields_}


def write_bracken(nodes, names, rows, level, path):
    """Bracken's output table (sh_k2_bracken_write; host only)"""
    r = np.ascontiguousarray(rows, dtype=BRACKEN_ROW_DTYPE)
    S.check(S.load().sh_k2_bracken_write(nodes, C.c_uint64(len(nodes)), names, C.c_uint64(len(names)), C.c_void_p(r.ctypes.data), C.c_uint64(len(r)),
                                         C.c_int32(ord(level)), None if path is None else str(path).encode()))


def build_kmer_distrib(db_dir, inputs, read_len, seqid2taxid=None, taxid=0, output=None, chunk_bytes=0, device=0):
    """`scrubby-hip k2-bracken-build` (sh_k2_distrib_run): the k-mer distribution of a database directory at one read length over
    library FASTA files, written to `output` or <db>/database<L>mers.kmer_distrib; returns the result fields as a dict."""
    S.require_gpu()
    c = K2DistribConfig()
    files = [inputs] if isinstance(inputs, (str, bytes)) or hasattr(inputs, "__fspath__") else list(inputs)
    arr = (C.c_char_p * len(files))(*[str(f).encode() for f in files])
    c.db, c.input, c.n_input, c.read_len = str(db_dir).encode(), arr, len(files), read_len
    c.seqid2taxid = str(seqid2taxid).encode() if seqid2taxid else None
    c.taxid, c.output, c.chunk_bytes, c.device = taxid, str(output).encode() if output else None, chunk_bytes, device
    r = K2DistribResult()
    S.check(S.load().sh_k2_distrib_run(C.byref(c), C.byref(r)))
    return {n: getattr(r, n) for n, _ in K2DistribResult._fields_}


def bracken(db_dir, report, output, read_len=0, level="S", threshold=10, kmer_distrib=None):
    """`scrubby-hip k2-bracken` (sh_k2_bracken_run; host only): re-estimates one sample from its kraken.report; returns the
    summary fields, n_report_rows and n_unknown_taxa as a dict."""
    c = K2BrackenConfig()
    c.db, c.report, c.output = str(db_dir).encode(), str(report).encode(), str(output).encode()
    c.read_len, c.level, c.threshold = read_len, ord(level), threshold
    c.kmer_distrib = str(kmer_distrib).encode() if kmer_distrib else None
    r = K2BrackenResult()
    S.check(S.load().sh_k2_bracken_run(C.byref(c), C.byref(r)))
    out = {n: getattr(r.summary, n) for n, _ in K2BrackenSummary._fields_}
    out.update(n_report_rows=r.n_report_rows, n_unknown_taxa=r.n_unknown_taxa)
    return out


class K2Db:
    def __init__(self, handle):
        self.h = handle

    @classmethod
    def open(cls, path, device=0):
        S.require_gpu()
        h = C.c_void_p()
        S.check(S.load().sh_k2_open(str(path).encode(), device, C.byref(h)))
        return cls(h)

    @classmethod
    def create(cls, opts, capacity, parents, externals, names, ranks, device=0):
        S.require_gpu()
        nodes, npool, rpool = make_taxonomy(parents, externals, names, ranks)
        h = C.c_void_p()
        S.check(S.load().sh_k2_create(C.byref(opts), C.c_uint64(capacity), nodes, C.c_uint64(len(parents)), npool, C.c_uint64(len(npool)),
                                      rpool, C.c_uint64(len(rpool)), device, C.byref(h)))
        return cls(h)

    def insert(self, keys, taxa):
        import torch
        dk = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64)).cuda()
        dt = torch.from_numpy(np.ascontiguousarray(taxa, dtype=np.uint32).view(np.int32)).cuda()
        S.check(S.load().sh_k2_insert_device(self.h, C.c_void_p(dk.data_ptr()), C.c_void_p(dt.data_ptr()), C.c_uint64(len(keys)), None))

    def insert_sequence_device(self, d_bases, n, taxon):
        r = C.c_uint64()
        S.check(S.load().sh_k2_insert_sequence_device(self.h, C.c_void_p(d_bases.data_ptr()), C.c_uint64(n), C.c_uint32(taxon), None, C.byref(r)))
        return r.value

    def insert_sequence(self, seq, taxon):
        import torch
        a = np.frombuffer(bytes(seq), dtype=np.uint8) if not isinstance(seq, np.ndarray) else seq
        d = torch.from_numpy(np.concatenate([a, np.full(64, ord("N"), np.uint8)])).cuda()
        return self.insert_sequence_device(d, len(a), taxon)

    @classmethod
    def create_from_taxonomy(cls, opts, capacity, taxonomy, device=0):
        """an empty table over a Taxonomy; opts.value_bits is set from it"""
        S.require_gpu()
        nodes, npool, rpool = taxonomy.arrays()
        opts.value_bits = taxonomy.info()["value_bits"]
        h = C.c_void_p()
        S.check(S.load().sh_k2_create(C.byref(opts), C.c_uint64(capacity), nodes, C.c_uint64(len(nodes)), npool, C.c_uint64(len(npool)),
                                      rpool, C.c_uint64(len(rpool)), device, C.byref(h)))
        return cls(h)

    def set_min_acceptable_hash(self, v):
        S.check(S.load().sh_k2_set_min_acceptable_hash(self.h, C.c_uint64(v)))

    def insert_library_device(self, d_bases, d_offsets, d_taxa, n_records):
        """sh_k2_insert_library_device on torch tensors (uint8 bases readable 8 bytes past the end, int64 offsets, int32 taxa)"""
        st = K2BuildStats()
        S.check(S.load().sh_k2_insert_library_device(self.h, C.c_void_p(d_bases.data_ptr()), C.c_void_p(d_offsets.data_ptr()),
                                                     C.c_void_p(d_taxa.data_ptr()), C.c_uint64(n_records), S._stream_ptr(), C.byref(st)))
        return {n: getattr(st, n) for n, _ in K2BuildStats._fields_}

    def insert_library(self, records, taxa):
        """One launch over a list of sequences, record i under internal taxon taxa[i] (0 = skip)."""
        import torch
        assert len(records) == len(taxa)
        d_bases, d_off, n = _library_to_device(records)
        d_taxa = torch.from_numpy(np.ascontiguousarray(taxa, dtype=np.uint32).view(np.int32).copy()).cuda() if n else torch.zeros(1, dtype=torch.int32).cuda()
        return self.insert_library_device(d_bases, d_off, d_taxa, n)

    def insert_random(self, seed, n, taxon_lo, taxon_hi):
        S.check(S.load().sh_k2_insert_random(self.h, C.c_uint64(seed), C.c_uint64(n), C.c_uint32(taxon_lo), C.c_uint32(taxon_hi), None))

    def save(self, path):
        S.check(S.load().sh_k2_save(self.h, str(path).encode()))

    def info(self):
        i = K2Info()
        S.check(S.load().sh_k2_info_get(self.h, C.byref(i)))
        return {n: getattr(i, n) for n, _ in K2Info._fields_}

    def opts(self):
        o = K2Opts()
        S.check(S.load().sh_k2_db_opts(self.h, C.byref(o)))
        return o

    def export(self):
        i = self.info()
        cells = np.zeros(i["capacity"], dtype=np.uint32)
        parent = np.zeros(i["n_nodes"], dtype=np.uint32)
        ext = np.zeros(i["n_nodes"], dtype=np.uint32)
        S.check(S.load().sh_k2_export(self.h, C.c_void_p(cells.ctypes.data), C.c_void_p(parent.ctypes.data), C.c_void_p(ext.ctypes.data)))
        return cells, parent, ext

    def _classify(self, device, opts, batch, out_ptr, want_hits, minimizer_data):
        """the one call behind classify (device=False: sh_k2_classify_ex_batch) and classify_device / classify_device_hits
        (sh_k2_classify_ex_device on torch's current stream): (stats, the hits handle or None)"""
        L = S.load()
        st, h = K2Stats(), C.c_void_p()
        head = (self.h, C.byref(opts) if opts is not None else None, C.byref(batch), C.c_void_p(out_ptr))
        tail = (C.byref(st), C.byref(h) if want_hits else None, minimizer_data.h if minimizer_data is not None else None)
        S.check(L.sh_k2_classify_ex_device(*head, S._stream_ptr(), *tail) if device else L.sh_k2_classify_ex_batch(*head, *tail))
        return _stats_dict(st), h if want_hits else None

    def classify(self, bases, offsets, paired=False, opts=None, quals=None, hits=False, minimizer_data=None):
        """sh_k2_classify_ex_batch.
        quals (optional): Phred+33 bytes at the offsets of `bases` (0xFF = never masked), used when opts.min_base_quality > 0.
        hits=True: also Kraken 2's hit lists, returned third as (offsets, entries): unit i's entries (HIT_DTYPE) are
        entries[offsets[i]:offsets[i + 1]].
        minimizer_data: a MinimizerData the call adds to; the return values are the same."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
            assert len(quals) >= int(offsets[-1]), "one quality byte per base"
        n_rec = len(offsets) - 1
        n_units = n_rec // 2 if paired else n_rec
        out = np.zeros(max(n_units, 1), dtype=RESULT_DTYPE)
        b = K2Batch(bases.ctypes.data, quals.ctypes.data if quals is not None else None, offsets.ctypes.data, n_rec, 1 if paired else 0)
        stats, h = self._classify(False, opts, b, out.ctypes.data, hits, minimizer_data)
        if not hits:
            return out[:n_units], stats
        offs, ent, stats["n_hits_redone"] = _take_hits(h)
        return out[:n_units], stats, (offs, ent)

    def classify_hit_strings(self, bases, offsets, paired=False, opts=None, quals=None):
        """results, stats and column 5 of kraken.reads for every unit (strings, external taxids)"""
        out, st, (offs, ent) = self.classify(bases, offsets, paired=paired, opts=opts, quals=quals, hits=True)
        ext = self.export_external()
        return out, st, [format_hits(ent[int(offs[i]): int(offs[i + 1])], ext) for i in range(len(out))]

    def export_external(self):
        ext = np.zeros(self.info()["n_nodes"], dtype=np.uint32)
        S.check(S.load().sh_k2_export(self.h, None, None, C.c_void_p(ext.ctypes.data)))
        return ext

    def classify_device_hits(self, d_bases, d_offsets, n_records, paired, d_out, opts=None, d_quals=None, to_host=True, minimizer_data=None):
        """sh_k2_classify_ex_device with hit lists: results into d_out; returns (stats, (offsets, entries)) copied to the host, or
        with to_host=False (stats, (d_offsets_ptr, d_entries_ptr, n_units, n_entries, handle)) - free the handle with free_hits.
        minimizer_data: a MinimizerData the call adds to."""
        b = K2Batch(d_bases.data_ptr(), d_quals.data_ptr() if d_quals is not None else None, d_offsets.data_ptr(), n_records, 1 if paired else 0)
        stats, h = self._classify(True, opts, b, d_out.data_ptr(), True, minimizer_data)
        if to_host:
            offs, ent, stats["n_hits_redone"] = _take_hits(h)
            return stats, (offs, ent)
        nu, ne, po, pe = C.c_uint64(), C.c_uint64(), C.c_void_p(), C.c_void_p()
        S.check(S.load().sh_k2_hits_count(h, C.byref(nu), C.byref(ne), None))
        S.check(S.load().sh_k2_hits_device(h, C.byref(po), C.byref(pe)))
        return stats, (po.value, pe.value, nu.value, ne.value, h)

    @staticmethod
    def free_hits(h):
        S.load().sh_k2_hits_free(h)

    @staticmethod
    def hits_redone(h):
        r = C.c_uint64()
        S.check(S.load().sh_k2_hits_count(h, None, None, C.byref(r)))
        return r.value

    def classify_device(self, d_bases, d_offsets, n_records, paired, d_out, opts=None, d_quals=None, minimizer_data=None):
        """sh_k2_classify_ex_device without hit lists: results into d_out; returns the stats"""
        b = K2Batch(d_bases.data_ptr(), d_quals.data_ptr() if d_quals is not None else None, d_offsets.data_ptr(), n_records, 1 if paired else 0)
        return self._classify(True, opts, b, d_out.data_ptr(), False, minimizer_data)[0]

    def value_counts(self, return_stats=False):
        """minimizers of the table per internal taxon (sh_k2_value_counts): uint64[n_nodes]; with return_stats=True also the
        call's statistics (n_cells, n_occupied, n_bad_values, ms)"""
        counts = np.zeros(self.info()["n_nodes"], dtype=np.uint64)
        st = K2InspectStats()
        S.check(S.load().sh_k2_value_counts(self.h, C.c_void_p(counts.ctypes.data), C.byref(st)))
        return (counts, _inspect_stats(st)) if return_stats else counts

    def value_counts_device(self, d_counts, stream=None, stats=False):
        """sh_k2_value_counts_device into d_counts (a torch int64 tensor of n_nodes elements on the database's device, overwritten)
        on `stream` (a torch stream; None: the current one).  Without stats the call only enqueues; with stats=True it waits and
        returns the statistics."""
        assert d_counts.numel() >= self.info()["n_nodes"] and d_counts.element_size() == 8 and d_counts.is_contiguous()
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else S._stream_ptr()
        st = K2InspectStats() if stats else None
        S.check(S.load().sh_k2_value_counts_device(self.h, C.c_void_p(d_counts.data_ptr()), sp, C.byref(st) if stats else None))
        return _inspect_stats(st) if stats else None

    def inspect_header(self):
        """the seven '#' lines kraken2-inspect prints in front of its report (sh_k2_inspect_header)"""
        n = C.c_uint64()
        S.check(S.load().sh_k2_inspect_header(self.h, None, C.c_uint64(0), C.byref(n)))
        buf = C.create_string_buffer(n.value + 1)
        S.check(S.load().sh_k2_inspect_header(self.h, buf, C.c_uint64(n.value + 1), C.byref(n)))
        return buf.value.decode()

    def write_report(self, results, path):
        r = np.ascontiguousarray(results, dtype=RESULT_DTYPE)
        S.check(S.load().sh_k2_write_report(self.h, C.c_void_p(r.ctypes.data), C.c_uint64(len(r)), str(path).encode()))

    def write_minimizer_report(self, results, minimizer_data, path):
        """the 8-column report of kraken2 --report-minimizer-data from per-unit results and a MinimizerData"""
        r = np.ascontiguousarray(results, dtype=RESULT_DTYPE)
        S.check(S.load().sh_k2_mindata_write_report(self.h, C.c_void_p(r.ctypes.data), C.c_uint64(len(r)), minimizer_data.h, str(path).encode()))

    def close(self):
        if self.h:
            S.load().sh_k2_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kraken_run(inputs, outputs, db, taxa=(), taxa_direct=(), workdir=None, confidence=-1.0, min_hit_groups=0, extract=False,
               json=None, read_ids=None, command="", device=0, threads=4, classifier_args=None, min_base_quality=0, quick=False,
               report_minimizer_data=False):
    c = KrakenConfig()
    for i, (a, b) in enumerate(zip(inputs, outputs)):
        c.input[i], c.output[i] = str(a).encode(), str(b).encode()
    c.n_files, c.extract, c.db = len(inputs), int(extract), str(db).encode()
    c.workdir = str(workdir).encode() if workdir else None
    ta = (C.c_char_p * max(len(taxa), 1))(*[t.encode() for t in taxa])
    td = (C.c_char_p * max(len(taxa_direct), 1))(*[t.encode() for t in taxa_direct])
    c.taxa, c.n_taxa, c.taxa_direct, c.n_taxa_direct = ta, len(taxa), td, len(taxa_direct)
    c.confidence, c.min_hit_groups = confidence, min_hit_groups
    c.json = str(json).encode() if json else None
    c.read_ids = str(read_ids).encode() if read_ids else None
    c.command, c.device, c.threads = command.encode(), device, threads
    c.classifier_args = classifier_args.encode() if classifier_args else None
    c.min_base_quality, c.quick, c.report_minimizer_data = min_base_quality, int(quick), int(bool(report_minimizer_data))
    r = S.ReadsResult()
    S.check(S.load().sh_kraken_run(C.byref(c), C.byref(r)))
    return {n: getattr(r, n) for n, _ in S.ReadsResult._fields_}
