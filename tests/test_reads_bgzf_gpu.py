"""SCRUBBY_HIP_GUNZIP_DEVICE=1 end to end: BGZF inputs of sh_reads_run and of Index.build_fasta are inflated on the device (shc::In in
sh_codec.h, the gz branch of sh_index.hip, sh_inflate.hip).  The outputs and counts must be those of the plain-input run; that the
members really went through the device - and no file fell back to zlib - is read from the `gunzip on the device` line of
SCRUBBY_HIP_DBG_HOST=1.  What the scan does not take (a plain gzip member behind BGZF ones) goes through zlib with one notice; a
truncated last member is an error with the switch on and off; with the switch unset or "0" nothing of this runs."""
import gzip
import re

import numpy as np
import pytest

from tests import bgzf_util as B
from tests.test_reads_e2e_gpu import dataset      # noqa: F401  (10 k pairs against 5 Mb)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
COUNTS = ("reads_in", "reads_out", "reads_removed", "reads_extracted", "n_depleted_ids")
NOTICE = "SCRUBBY_HIP_GUNZIP_DEVICE:"


def _gunzip_line(err):
    """(members, bytes out, files through zlib) of the one line a run prints, or None"""
    got = re.findall(r"gunzip on the device: (\d+) members, (\d+) bytes out, (\d+) files through zlib", err)
    assert len(got) <= 1, err
    return tuple(int(v) for v in got[0]) if got else None


@pytest.fixture(scope="module")
def files(dataset):
    d, fa, r1, r2, ids, n_pairs = dataset
    t1, t2 = open(r1, "rb").read(), gzip.open(r2, "rb").read()
    b1, b2, p2 = d / "B1.fastq.gz", d / "B2.fastq.gz", d / "P2.fastq"
    b1.write_bytes(B.bgzf(t1))
    b2.write_bytes(B.bgzf(t2, level=1))
    p2.write_bytes(t2)
    return t1, t2, str(b1), str(b2), str(p2)


@pytest.fixture(scope="module")
def plain_run(dataset, files):
    from scrubby_amd import lib as S
    d, fa, r1, r2, ids, n_pairs = dataset
    t1, t2, b1, b2, p2 = files
    o1, o2 = str(d / "bgp_1.fastq"), str(d / "bgp_2.fastq")
    res = S.reads_run([r1, p2], [o1, o2], fa, json=str(d / "bgp.json"), threads=6)
    return open(o1, "rb").read(), open(o2, "rb").read(), res


def test_switch_unset_or_zero_changes_nothing(dataset, files, plain_run, monkeypatch, capfd):
    """first in the file: no inflater exists in the process yet, so the run's device memory would show one (224 MiB of staging)"""
    import torch
    from scrubby_amd import lib as S
    d, fa, r1, r2, ids, n_pairs = dataset
    t1, t2, b1, b2, p2 = files
    p1, pp2, pres = plain_run
    monkeypatch.setenv("SCRUBBY_HIP_DBG_HOST", "1")
    o1, o2 = str(d / "bgu_1.fastq"), str(d / "bgu_2.fastq")
    for value in (None, "0"):
        if value is None:
            monkeypatch.delenv("SCRUBBY_HIP_GUNZIP_DEVICE", raising=False)
        else:
            monkeypatch.setenv("SCRUBBY_HIP_GUNZIP_DEVICE", value)
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info()[0]
        capfd.readouterr()
        res = S.reads_run([b1, b2], [o1, o2], fa, json=str(d / "bgu.json"), threads=6)
        err = capfd.readouterr().err
        free_after = torch.cuda.mem_get_info()[0]
        assert _gunzip_line(err) is None and NOTICE not in err
        # a pooled inflater's device staging is 32 MiB of window + 192 MiB of output (sh_codec.h); a run's own scratch may grow by less
        assert free_before - free_after < (192 << 20), "device memory of the size of an inflater was taken"
        assert open(o1, "rb").read() == p1 and open(o2, "rb").read() == pp2
        assert [res[k] for k in COUNTS] == [pres[k] for k in COUNTS]


@pytest.mark.parametrize("chunk_mb", [None, "1"])
def test_reads_run_bgzf_inputs_equal_the_plain_run(dataset, files, plain_run, monkeypatch, capfd, chunk_mb):
    from scrubby_amd import lib as S
    d, fa, r1, r2, ids, n_pairs = dataset
    t1, t2, b1, b2, p2 = files
    p1, pp2, pres = plain_run
    monkeypatch.setenv("SCRUBBY_HIP_GUNZIP_DEVICE", "1")
    monkeypatch.setenv("SCRUBBY_HIP_DBG_HOST", "1")
    if chunk_mb:
        monkeypatch.setenv("SCRUBBY_HIP_CHUNK_MB", chunk_mb)      # each file is ~3.3 MB: chunks and members do not line up
    o1, o2 = str(d / f"bgd{chunk_mb}_1.fastq"), str(d / f"bgd{chunk_mb}_2.fastq")
    capfd.readouterr()
    res = S.reads_run([b1, b2], [o1, o2], fa, json=str(d / f"bgd{chunk_mb}.json"), threads=6)
    err = capfd.readouterr().err
    assert open(o1, "rb").read() == p1 and open(o2, "rb").read() == pp2
    assert [res[k] for k in COUNTS] == [pres[k] for k in COUNTS] and res["reads_removed"] == 2 * len(ids)
    members, out_bytes, through_zlib = _gunzip_line(err)
    print(err.strip().splitlines()[-1])
    # What a run reads of its inputs is fixed: the emptiness check opens each file for one byte, which inflates the reader's first window
    # (the whole members inside the first 256 KiB of the file), and pass 1 then reads each file once from its start; pass 2 filters the
    # chunks pass 1 kept.  So the line shows every member of both files once, plus each file's first window - a window inflated twice,
    # or a member missed, would show.
    want_members, want_bytes = B.n_members(t1) + B.n_members(t2), len(t1) + len(t2)
    for path in (b1, b2):
        first, used, stopped = S.bgzf_scan(open(path, "rb").read()[:256 << 10])
        assert stopped == 1 and 0 < len(first) < B.n_members(t1)
        want_members += len(first)
        want_bytes += sum(m.out_len for m in first)
    assert (members, out_bytes, through_zlib) == (want_members, want_bytes, 0)
    assert NOTICE not in err


def test_index_from_a_bgzf_reference(dataset, oracle, monkeypatch, capfd):
    from scrubby_amd import lib as S
    d, fa, r1, r2, ids, n_pairs = dataset
    text = gzip.open(fa, "rb").read()
    plain, bg = d / "ref_plain.fa", d / "ref_bgzf.fa.gz"
    plain.write_bytes(text)
    bg.write_bytes(B.bgzf(text))
    want = S.Index.build_fasta(str(plain), S.preset("sr"))
    monkeypatch.setenv("SCRUBBY_HIP_GUNZIP_DEVICE", "1")
    monkeypatch.setenv("SCRUBBY_HIP_DBG_HOST", "1")
    capfd.readouterr()
    got = S.Index.build_fasta(str(bg), S.preset("sr"))
    err = capfd.readouterr().err
    assert _gunzip_line(err) == (B.n_members(text), len(text), 0) and NOTICE not in err
    wi, gi = want.info(), got.info()
    for k in wi:
        if k != "build_ms":
            assert wi[k] == gi[k], k
    for a, b in zip(want.export_ref(), got.export_ref()):
        assert np.array_equal(a, b)
    # the table's content (a slot's place depends on the order the insertions won their races: compare the dumps, as test_index_mmi.py does)
    dumps = [oracle.Index.wrap(*i.export(), wi["w"], wi["k"]).dump() for i in (want, got)]
    assert all(np.array_equal(a, b) for a, b in zip(*dumps))


def test_a_plain_gzip_member_behind_bgzf_ones_goes_through_zlib(dataset, files, plain_run, monkeypatch, capfd):
    from scrubby_amd import lib as S
    d, fa, r1, r2, ids, n_pairs = dataset
    t1, t2, b1, b2, p2 = files
    p1, pp2, pres = plain_run
    mixed = d / "M1.fastq.gz"
    mixed.write_bytes(B.member(t1[:60000]) + B.member(t1[60000:120001]) + gzip.compress(t1[120001:]))
    monkeypatch.setenv("SCRUBBY_HIP_GUNZIP_DEVICE", "1")
    monkeypatch.setenv("SCRUBBY_HIP_DBG_HOST", "1")
    o1, o2 = str(d / "bgm_1.fastq"), str(d / "bgm_2.fastq")
    capfd.readouterr()
    res = S.reads_run([str(mixed), p2], [o1, o2], fa, json=str(d / "bgm.json"), threads=6)
    err = capfd.readouterr().err
    assert open(o1, "rb").read() == p1 and open(o2, "rb").read() == pp2
    assert [res[k] for k in COUNTS] == [pres[k] for k in COUNTS]
    members, out_bytes, through_zlib = _gunzip_line(err)
    assert members >= 2 and through_zlib >= 1
    assert err.count(NOTICE) == 1 and "not BGZF" in err      # announced once, whatever number of readers met it


def test_an_empty_bgzf_file_is_an_empty_gz(dataset, monkeypatch, tmp_path):
    from scrubby_amd import lib as S
    d, fa, r1, r2, ids, n_pairs = dataset
    results = {}
    for name, content, env in (("gz", gzip.compress(b""), None), ("bgzf", B.EOF, "1")):
        src = tmp_path / f"empty_{name}.fastq.gz"
        src.write_bytes(content)
        if env:
            monkeypatch.setenv("SCRUBBY_HIP_GUNZIP_DEVICE", env)
        out = tmp_path / f"out_{name}.fastq"
        try:
            res = S.reads_run([str(src)], [str(out)], fa, preset="sr", json=str(tmp_path / f"{name}.json"))
            results[name] = ([res[k] for k in COUNTS], out.read_bytes() if out.exists() else None)
        except S.ScrubbyHipError as e:
            results[name] = (e.status, None)
    assert results["bgzf"] == results["gz"]


@pytest.mark.parametrize("switch", [None, "1"])
def test_a_truncated_last_member_is_an_error(dataset, files, monkeypatch, tmp_path, switch):
    from scrubby_amd import lib as S
    d, fa, r1, r2, ids, n_pairs = dataset
    t1, t2, b1, b2, p2 = files
    cut = tmp_path / "cut.fastq.gz"
    cut.write_bytes(open(b1, "rb").read()[:-40])      # the end-of-file member and 12 bytes of the last data member are gone
    if switch:
        monkeypatch.setenv("SCRUBBY_HIP_GUNZIP_DEVICE", switch)
    else:
        monkeypatch.delenv("SCRUBBY_HIP_GUNZIP_DEVICE", raising=False)
    with pytest.raises(S.ScrubbyHipError) as e:
        S.reads_run([str(cut)], [str(tmp_path / "o.fastq")], fa, preset="sr", json=str(tmp_path / "o.json"))
    assert e.value.status == 7
