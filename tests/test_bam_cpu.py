"""`scrubby alignment` on SAM and BAM, the host side: sh_bam_header, the host mirror sh_bam_filter_host against the plain model of
bam_util.py on every case of its table (one window, and windows cut at every offset), sh_alignment_run end to end, the bounds the
device path's tables rest on, and csrc/sh_bam.h under the sanitizers in a program of its own.  No GPU."""
import ctypes
import gzip
import json
import os
import re
import subprocess

import pytest

from tests import bam_util as B
from scrubby_amd import lib as S

HERE = os.path.dirname(os.path.abspath(__file__))
SEG, CAP = S.bam_segment(), S.bam_segment_cap()
CASES = B.cases(SEG, CAP)
CORRUPT = B.corrupt_cases(SEG)


def names_of(case, r, **kw):
    return S.bam_filter_host(case.text, case.n_ref, entry=kw.pop("entry", case.first), **r, **kw)


def test_constants_match_the_header():
    src = open(os.path.join(HERE, "..", "scrubby_amd", "csrc", "sh_bam.h")).read()
    assert int(re.search(r"#define SHB_LANE_CIGAR (\d+)u", src).group(1)) == B.LANE_CIGAR
    assert re.search(r"#define SHB_MAX_RECORD \(64u << 20\)", src) and B.MAX_RECORD == 64 << 20
    assert SEG % 64 == 0 and CAP >= 16


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.label)
def test_host_filter_matches_the_model(case):
    for r in case.rules:
        exp, counts = B.model(case.recs, r)
        names, nxt, st = names_of(case, r)
        assert names == exp, (case.label, r)
        assert nxt == len(case.text)
        for k, v in counts.items():
            assert st[k] == v, (case.label, r, k)
        assert st["n_segments"] == len({s // SEG for s in case.starts[:-1]})
    # some rule selects something and some rule leaves something out: the table decides
    sel = [B.model(case.recs, r)[1]["n_selected"] for r in case.rules]
    assert max(sel) > 0 and min(sel) < len(case.recs)


def test_entry_behind_the_first_record():
    case = CASES[1]
    for k in (1, 2):
        names, nxt, st = names_of(case, case.rules[0], entry=case.starts[k])
        assert names == B.model(case.recs[k:], case.rules[0])[0] and nxt == len(case.text) and st["n_records"] == len(case.recs) - k


@pytest.mark.parametrize("case", [c for c in CASES if c.label in ("fields", "coverage")], ids=lambda c: c.label)
def test_windows_cut_at_every_offset(case):
    r = case.rules[0]
    exp = B.model(case.recs, r)[0]
    text = case.text
    for cut in range(case.first, len(text) + 1):
        n1, nxt, _ = S.bam_filter_host(text[:cut], case.n_ref, entry=case.first, last=False, **r)
        assert nxt == max(s for s in case.starts if s <= cut), cut
        n2, end, _ = S.bam_filter_host(text[nxt:], case.n_ref, entry=0, last=True, base=nxt, **r)
        assert n1 + n2 == exp and end == len(text) - nxt, cut


@pytest.mark.parametrize("case", CASES[:3], ids=lambda c: c.label)
def test_window_ends(case):
    r = case.rules[0]
    for label, cut, complete in B.window_cuts(case):
        k = max(i for i, s in enumerate(case.starts) if s <= cut)
        names, nxt, _ = S.bam_filter_host(case.text[:cut], case.n_ref, entry=case.first, last=False, **r)
        assert names == B.model(case.recs[:k], r)[0] and nxt == case.starts[k], label
        if complete:
            assert S.bam_filter_host(case.text[:cut], case.n_ref, entry=case.first, last=True, **r)[0] == names
        else:
            with pytest.raises(S.ScrubbyHipError, match=f"truncated BAM record at {1000 + case.starts[k]}$"):
                S.bam_filter_host(case.text[:cut], case.n_ref, entry=case.first, last=True, base=1000, **r)


@pytest.mark.parametrize("case", CORRUPT, ids=lambda c: c.label)
def test_corrupt_records_are_named(case):
    for base in (0, 5 << 30):
        with pytest.raises(S.ScrubbyHipError, match=f"not a BAM record at {base + case.error_at}$"):
            S.bam_filter_host(case.text, case.n_ref, entry=case.first, base=base, **case.rules[0])


def test_arguments_are_refused_by_name():
    case = CASES[0]
    with pytest.raises(S.ScrubbyHipError, match="room for 10 name bytes"):
        S.bam_filter_host(case.text, case.n_ref, entry=case.first, names_cap=10)
    with pytest.raises(S.ScrubbyHipError, match="entry"):
        S.bam_filter_host(case.text, case.n_ref, entry=len(case.text) + 1, names_cap=1 << 20)


def test_header():
    for n_ref in (0, 3):
        h = B.header(n_ref)
        assert S.bam_header(h) == (0, n_ref, len(h))
        assert S.bam_header(h + b"\x25\0\0\0rest") == (0, n_ref, len(h))
        for cut in range(len(h)):
            assert S.bam_header(h[:cut])[0] == 1, cut
    assert S.bam_header(b"BAM\2" + B.header(1)[4:])[0] == 2
    assert S.bam_header(b"r1\t0\tchr1\t1\t60\t4M\t*\t0\t0\tACGT\t*\n")[0] == 2
    assert S.bam_header(b"\x1f\x8b\x08\x04")[0] == 2
    assert S.bam_header(b"BA")[0] == 1 and S.bam_header(b"")[0] == 1


def test_table_bounds():
    """What k_bam_probe's tables rest on: the ordinary cases hold at most 16 positions per segment at which a record may start, the
    flood holds more than the table's cap in a segment the chain enters."""
    for case in CASES:
        counts = S.bam_plausible_counts(case.text, case.n_ref)
        assert len(counts) == -(-len(case.text) // SEG)
        if not case.flood:
            assert int(counts.max()) <= 16, (case.label, counts.tolist())
        else:
            entered = {s // SEG for s in case.starts[:-1]}
            assert any(int(counts[s]) > CAP for s in entered), counts.tolist()
    for case in CORRUPT:
        assert int(S.bam_plausible_counts(case.text, case.n_ref).max()) <= 16


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
E2E = [B.aligned(b"r1", 150), B.Rec(name=b"r2", cigar=((B.S, 100), (B.M, 50))),B.aligned(b"r3", 150, mapq=3), B.aligned(b"r4", 150, flag=4),
       B.Rec(name=b"r2", cigar=((B.S, 30), (B.M, 120)), mapq=20), B.Rec(name=b"r6", cigar=((B.M, 70), (B.I, 10), (B.D, 5), (B.EQ, 70)), mapq=40)]
E2E_RULES = [dict(min_len=0, min_cov=0.0, min_mapq=0), dict(min_len=100, min_cov=2.0, min_mapq=0), dict(min_len=1000, min_cov=0.5, min_mapq=30), dict(min_len=80, min_cov=2.0, min_mapq=30)]


def fastq(tmp_path):
    fq = tmp_path / "r.fq"
    fq.write_text("".join(f"@r{i} x\nACGT\n+\nIIII\n" for i in range(1, 8)))
    return fq


def run(tmp_path, aln, r, tag, **kw):
    out = tmp_path / f"o_{tag}.fq"
    res = S.alignment_run([str(fastq(tmp_path))], [str(out)], str(aln), **r, **kw)
    kept = [l[1:].split()[0] for l in out.read_text().split("\n") if l.startswith("@")] if out.exists() else []
    return res, kept


@pytest.mark.parametrize("r", E2E_RULES)
def test_alignment_run_on_bam_and_sam(tmp_path, r):
    exp = {x.name.decode() for x in E2E if B.selects(x, r)}
    bam = tmp_path / "aln.bam"; bam.write_bytes(B.bam_file(3, E2E, block=300))
    sam = tmp_path / "aln.sam"; sam.write_text(B.sam_text(3, E2E))
    as_sam = tmp_path / "holds_bam.sam"; as_sam.write_bytes(B.bam_file(3, E2E))
    samgz = tmp_path / "aln.sam.gz"
    with gzip.open(samgz, "wt") as f:
        f.write(B.sam_text(3, E2E))
    odd = tmp_path / "aln.dat"; odd.write_bytes(B.bam_file(3, E2E))
    for tag, aln, kw in [("bam", bam, {}), ("sam", sam, {}), ("holds_bam", as_sam, {}), ("samgz", samgz, dict(fmt="sam")), ("fmt_bam", odd, dict(fmt="bam")),
                         ("sam_as_bam", sam, dict(fmt="bam"))]:
        res, kept = run(tmp_path, aln, r, tag, **kw)
        assert res["n_depleted_ids"] == len(exp), tag
        assert kept == [f"r{i}" for i in range(1, 8) if f"r{i}" not in exp], tag
    res, kept = run(tmp_path, bam, r, "extract", extract=True)
    assert kept == [f"r{i}" for i in range(1, 8) if f"r{i}" in exp]


def test_json_settings_and_formats(tmp_path):
    bam = tmp_path / "aln.bam"; bam.write_bytes(B.bam_file(3, E2E))
    js = tmp_path / "rep.json"
    run(tmp_path, bam, dict(min_len=100, min_cov=0.25, min_mapq=7), "js", json=str(js))
    st = json.load(open(js))["settings"]
    assert st["alignment"] == str(bam) and st["min_len"] == 100 and st["min_cov"] == 0.25 and st["min_mapq"] == 7 and st["aligner"] is None
    cram = tmp_path / "aln.cram"; cram.write_bytes(b"CRAM\3\0")
    for kw in (dict(), dict(fmt="cram")):
        with pytest.raises(S.ScrubbyHipError, match="(?i)AlignmentInputFormatInvalid.*cram"):
            run(tmp_path, cram, {}, "cram", **kw)
    with pytest.raises(S.ScrubbyHipError, match="AlignmentInputFormatNotRecognized"):
        run(tmp_path, tmp_path / "aln.sam.gz", {}, "gz")


def test_a_bam_larger_than_a_window_of_the_host_path(tmp_path):
    """Records of 40 KB, 20 MB in all: the host path carries a tail from window to window."""
    recs = [B.Rec(name=b"w%d" % i, cigar=((B.M, 27000),), mapq=i % 61) for i in range(500)]
    bam = tmp_path / "big.bam"; bam.write_bytes(B.bam_file(3, recs))
    fq = tmp_path / "w.fq"; fq.write_text("".join(f"@w{i}\nAC\n+\nII\n" for i in range(0, 500, 7)))
    res = S.alignment_run([str(fq)], [str(tmp_path / "w_out.fq")], str(bam), min_mapq=30)
    assert res["n_depleted_ids"] == sum(1 for r in recs if r.mapq >= 30)


@pytest.mark.parametrize("label,text", [
    ("few_fields", "r1\t0\tchr1\t1\t60\t4M\n"),
    ("hex_flag", "r1\t0x10\tchr1\t1\t60\t4M\t*\t0\t0\tACGT\t*\n"),
    ("mapq", "r1\t0\tchr1\t1\t256\t4M\t*\t0\t0\tACGT\t*\n"),
    ("cigar_op", "r1\t0\tchr1\t1\t60\t4Q\t*\t0\t0\tACGT\t*\n"),
    ("cigar_no_length", "r1\t0\tchr1\t1\t60\tM\t*\t0\t0\tACGT\t*\n"),
    ("cigar_seq_differ", "r1\t0\tchr1\t1\t60\t5M\t*\t0\t0\tACGT\t*\n"),
])
def test_sam_errors_name_the_line(tmp_path, label, text):
    sam = tmp_path / "bad.sam"; sam.write_text("@HD\tVN:1.6\nok\t0\tchr1\t1\t60\t4M\t*\t0\t0\tACGT\t*\n" + text)
    with pytest.raises(S.ScrubbyHipError, match="line 3"):
        run(tmp_path, sam, {}, label)


def test_sam_star_fields(tmp_path):
    sam = tmp_path / "star.sam"
    sam.write_text("a\t0\tchr1\t1\t60\t*\t*\t0\t0\tACGT\t*\nb\t0\tchr1\t1\t60\t4M\t*\t0\t0\t*\t*\nc\t0\tchr1\t1\t60\t2S2M\t*\t0\t0\tACGT\tIIII\tNM:i:0\n")
    # a: no ops, qalen 0; b: SEQ * -> qlen 0, coverage 0, qalen 4; c: qalen 2 of 4
    assert run(tmp_path, sam, dict(min_len=10 ** 6, min_cov=0.5), "s1")[0]["n_depleted_ids"] == 1
    assert run(tmp_path, sam, dict(min_len=4, min_cov=2.0), "s2")[0]["n_depleted_ids"] == 1
    assert run(tmp_path, sam, dict(min_len=10 ** 6, min_cov=0.0), "s3")[0]["n_depleted_ids"] == 3


def test_corrupt_bam_file_is_an_error(tmp_path):
    case = CORRUPT[0]
    bam = tmp_path / "bad.bam"; bam.write_bytes(B.bgzf(case.text))
    with pytest.raises(S.ScrubbyHipError, match=f"not a BAM record at {case.error_at}"):
        run(tmp_path, bam, {}, "bad")
    cut = tmp_path / "cut.bam"; cut.write_bytes(B.bgzf(CASES[0].text[:-5]))
    with pytest.raises(S.ScrubbyHipError, match="truncated BAM record"):
        run(tmp_path, cut, {}, "cut")


def test_cli_takes_sam_and_bam(tmp_path):
    exe = os.path.join(HERE, "..", "scrubby_amd", "scrubby-hip")
    bam = tmp_path / "aln.bam"; bam.write_bytes(B.bam_file(3, E2E))
    odd = tmp_path / "aln.bin"; odd.write_text(B.sam_text(3, E2E))
    exp = {x.name.decode() for x in E2E if B.selects(x, E2E_RULES[1])}
    for tag, aln, extra in (("bam", bam, []), ("sam", odd, ["--format", "sam"])):
        out = tmp_path / f"cli_{tag}.fq"
        subprocess.check_call([exe, "alignment", "-i", str(fastq(tmp_path)), "-o", str(out), "-a", str(aln), "-l", "100", "-c", "2.0"] + extra, stderr=subprocess.DEVNULL)
        assert [l[1:].split()[0] for l in out.read_text().split("\n") if l.startswith("@")] == [f"r{i}" for i in range(1, 8) if f"r{i}" not in exp]
    assert subprocess.run([exe, "alignment", "-i", str(fastq(tmp_path)), "-o", str(tmp_path / "x.fq"), "-a", str(bam), "--format", "cram"], capture_output=True).returncode != 0


# ---- the sanitizers and the symbols ----------------------------------------------------------------------------------------------------------
def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """tests/bam_host.cpp has its own main: shb_header, shb_walk and the plausible-position count over the table's valid and corrupt
    bytes, every prefix of the small ones included, each on a heap block of exactly the window's extent.  Built with AddressSanitizer
    and UBSan, runtimes linked statically, and run as a program."""
    exe = str(tmp_path / "bam_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-o", exe, os.path.join(HERE, "bam_host.cpp")])
    blob = tmp_path / "cases.bin"
    with open(blob, "wb") as f:      # n_ref, first, every-prefix flag, length, bytes
        for c in CASES + CORRUPT:
            small = len(c.text) < 6000
            f.write(ctypes.c_int32(c.n_ref)); f.write(ctypes.c_uint64(c.first)); f.write(ctypes.c_uint32(1 if small else 0)); f.write(ctypes.c_uint64(len(c.text))); f.write(c.text)
    out = subprocess.run([exe, str(blob)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"{len(CASES) + len(CORRUPT)} cases ok" in out.stdout


def test_abi_has_the_symbols():
    L = S.load()
    for name in ("sh_bam_header", "sh_bam_segment", "sh_bam_segment_cap", "sh_bam_names_bound", "sh_bam_scanner_create", "sh_bam_scanner_free", "sh_bam_filter_device",
                 "sh_bam_filter_host", "sh_bam_plausible_host"):
        assert hasattr(L, name) and name in S.EXPORTS
    assert L.sh_version() == 104
    assert S.bam_names_bound(0) >= 255 and S.bam_names_bound(291 * 10) >= 2550
