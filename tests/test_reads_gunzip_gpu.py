"""SCRUBBY_HIP_GUNZIP_DEVICE=2 end to end: ordinary .gz inputs (one long gzip member, what gzip and pigz write) of sh_reads_run and of
Index.build_fasta are inflated on the device through a sh_gunzip (shc::In in sh_codec.h, the gz branch of sh_index.hip, the k_gz_*
kernels of sh_inflate.hip).  Outputs and counts must be those of the plain-input run; that the bytes really went through the device -
and no file fell back to zlib - is read from the second sentence of the `gunzip on the device` line of SCRUBBY_HIP_DBG_HOST=1.  Under
"1" and with the switch unset nothing of this runs: no second sentence, and no device memory of the marker scratch's size."""
import gzip
import re

import numpy as np
import pytest

from tests import bgzf_util as B
from tests.test_reads_e2e_gpu import dataset      # noqa: F401  (10 k pairs against 5 Mb)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
COUNTS = ("reads_in", "reads_out", "reads_removed", "reads_extracted", "n_depleted_ids")
NOTICE = "SCRUBBY_HIP_GUNZIP_DEVICE:"


def _any_line(err):
    """(chunks, redone, bytes out, files through zlib) of the second sentence of the one line a run prints, or None"""
    got = re.findall(r"gunzip on the device: \d+ members, \d+ bytes out, \d+ files through zlib\. Any gzip stream: (\d+) chunks, (\d+) redone, (\d+) bytes out, (\d+) files through zlib", err)
    assert len(got) <= 1, err
    return tuple(int(v) for v in got[0]) if got else None


@pytest.fixture(scope="module")
def files(dataset):
    d, fa, r1, r2, ids, n_pairs = dataset
    t1, t2 = open(r1, "rb").read(), gzip.open(r2, "rb").read()
    g1, g2, p2 = d / "G1.fastq.gz", d / "G2.fastq.gz", d / "GP2.fastq"
    g1.write_bytes(gzip.compress(t1))
    g2.write_bytes(gzip.compress(t2, 1))
    p2.write_bytes(t2)
    return t1, t2, str(g1), str(g2), str(p2)


@pytest.fixture(scope="module")
def plain_run(dataset, files):
    from scrubby_amd import lib as S
    d, fa, r1, r2, ids, n_pairs = dataset
    t1, t2, g1, g2, p2 = files
    o1, o2 = str(d / "gzp_1.fastq"), str(d / "gzp_2.fastq")
    res = S.reads_run([r1, p2], [o1, o2], fa, json=str(d / "gzp.json"), threads=6)
    return open(o1, "rb").read(), open(o2, "rb").read(), res


@pytest.mark.parametrize("value", [None, "1"])
def test_unset_and_one_run_nothing_of_the_new_path(dataset, files, plain_run, monkeypatch, capfd, value):
    """first in the file: no sh_gunzip exists in the process yet, so its scratch (2 B per byte of a pooled inflater's 192 MiB of output)
    would show in the device memory"""
    import torch
    from scrubby_amd import lib as S
    d, fa, r1, r2, ids, n_pairs = dataset
    t1, t2, g1, g2, p2 = files
    p1, pp2, pres = plain_run
    monkeypatch.setenv("SCRUBBY_HIP_DBG_HOST", "1")
    if value is None:
        monkeypatch.delenv("SCRUBBY_HIP_GUNZIP_DEVICE", raising=False)
    else:
        monkeypatch.setenv("SCRUBBY_HIP_GUNZIP_DEVICE", value)
    o1, o2 = str(d / "gzu_1.fastq"), str(d / "gzu_2.fastq")
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    capfd.readouterr()
    res = S.reads_run([g1, g2], [o1, o2], fa, json=str(d / "gzu.json"), threads=6)
    err = capfd.readouterr().err
    free_after = torch.cuda.mem_get_info()[0]
    assert "Any gzip stream" not in err
    assert free_before - free_after < (384 << 20), "device memory of the size of the marker scratch was taken"
    assert open(o1, "rb").read() == p1 and open(o2, "rb").read() == pp2
    assert [res[k] for k in COUNTS] == [pres[k] for k in COUNTS]


def test_reads_run_on_ordinary_gz_inputs_equals_the_plain_run(dataset, files, plain_run, monkeypatch, capfd):
    from scrubby_amd import lib as S
    d, fa, r1, r2, ids, n_pairs = dataset
    t1, t2, g1, g2, p2 = files
    p1, pp2, pres = plain_run
    monkeypatch.setenv("SCRUBBY_HIP_GUNZIP_DEVICE", "2")
    monkeypatch.setenv("SCRUBBY_HIP_DBG_HOST", "1")
    o1, o2 = str(d / "gzd_1.fastq"), str(d / "gzd_2.fastq")
    capfd.readouterr()
    res = S.reads_run([g1, g2], [o1, o2], fa, json=str(d / "gzd.json"), threads=6)
    err = capfd.readouterr().err
    assert open(o1, "rb").read() == p1 and open(o2, "rb").read() == pp2
    assert [res[k] for k in COUNTS] == [pres[k] for k in COUNTS] and res["reads_removed"] == 2 * len(ids)
    chunks, redone, out_bytes, through_zlib = _any_line(err)
    print(err.strip().splitlines()[-1])
    assert through_zlib == 0 and NOTICE not in err
    assert chunks > 2 and out_bytes >= len(t1) + len(t2)      # pass 1 reads each file once from its start; the emptiness check reads a first window besides


def test_a_plain_member_behind_bgzf_ones_stays_on_the_device(dataset, files, plain_run, monkeypatch, capfd):
    from scrubby_amd import lib as S
    d, fa, r1, r2, ids, n_pairs = dataset
    t1, t2, g1, g2, p2 = files
    p1, pp2, pres = plain_run
    mixed = d / "GM1.fastq.gz"
    mixed.write_bytes(B.member(t1[:60000]) + B.member(t1[60000:120001]) + gzip.compress(t1[120001:]))
    monkeypatch.setenv("SCRUBBY_HIP_GUNZIP_DEVICE", "2")
    monkeypatch.setenv("SCRUBBY_HIP_DBG_HOST", "1")
    o1, o2 = str(d / "gzm_1.fastq"), str(d / "gzm_2.fastq")
    capfd.readouterr()
    res = S.reads_run([str(mixed), p2], [o1, o2], fa, json=str(d / "gzm.json"), threads=6)
    err = capfd.readouterr().err
    assert open(o1, "rb").read() == p1 and open(o2, "rb").read() == pp2
    assert [res[k] for k in COUNTS] == [pres[k] for k in COUNTS]
    chunks, redone, out_bytes, through_zlib = _any_line(err)
    assert NOTICE not in err and through_zlib == 0 and out_bytes >= len(t1) - 120001


def test_index_from_an_ordinary_gz_reference(dataset, oracle, monkeypatch, capfd):
    from scrubby_amd import lib as S
    d, fa, r1, r2, ids, n_pairs = dataset
    text = gzip.open(fa, "rb").read()
    plain, gzp = d / "gref_plain.fa", d / "gref.fa.gz"
    plain.write_bytes(text)
    gzp.write_bytes(gzip.compress(text, 6))
    want = S.Index.build_fasta(str(plain), S.preset("sr"))
    monkeypatch.setenv("SCRUBBY_HIP_GUNZIP_DEVICE", "2")
    monkeypatch.setenv("SCRUBBY_HIP_DBG_HOST", "1")
    capfd.readouterr()
    got = S.Index.build_fasta(str(gzp), S.preset("sr"))
    err = capfd.readouterr().err
    chunks, redone, out_bytes, through_zlib = _any_line(err)
    assert out_bytes == len(text) and through_zlib == 0 and NOTICE not in err
    wi, gi = want.info(), got.info()
    for k in wi:
        if k != "build_ms":
            assert wi[k] == gi[k], k
    for a, b in zip(want.export_ref(), got.export_ref()):
        assert np.array_equal(a, b)
    dumps = [oracle.Index.wrap(*i.export(), wi["w"], wi["k"]).dump() for i in (want, got)]
    assert all(np.array_equal(a, b) for a, b in zip(*dumps))
