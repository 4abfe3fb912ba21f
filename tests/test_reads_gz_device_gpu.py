"""SCRUBBY_HIP_GZ_DEVICE=1 end to end: pass 2 of sh_reads_run / sh_kraken_run hands the chunks of .gz outputs to the device deflaters
(sh_stream.cpp, sh_deflate.hip).  The outputs must inflate to exactly what the plain run writes, the counts must not move, several chunks
must land as several members in order, an empty output is still one valid empty member, and with the switch unset the files are zlib's
level-6 members byte for byte, as before.  That the chunks really went through the device - and none fell back to zlib - is read from
the pass-2 line of SCRUBBY_HIP_DBG_HOST=1."""
import gzip
import re
import zlib

import numpy as np
import pytest

from tests.test_reads_e2e_gpu import dataset      # noqa: F401  (10 k pairs against 5 Mb)
from tests.test_k2_gpu import K, cfg1, db, tax    # noqa: F401  (the suite's small Kraken database)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
COUNTS = ("reads_in", "reads_out", "reads_removed", "reads_extracted", "n_depleted_ids")


def _device_chunks(err):
    """(chunks deflated on the device, chunks that fell back to zlib) summed over the runs whose stderr this is"""
    assert "SCRUBBY_HIP_GZ_DEVICE:" not in err, err      # the one-time fallback notice
    got = re.findall(r"pass 2 device deflate: \d+ deflaters, (\d+) chunks on the device, (\d+) through zlib", err)
    return sum(int(a) for a, _ in got), sum(int(b) for _, b in got)


@pytest.fixture(scope="module")
def plain_run(dataset):
    from scrubby_amd import lib as S
    d, fa, r1, r2, ids, n_pairs = dataset
    o1, o2 = str(d / "gzp_1.fastq"), str(d / "gzp_2.fastq")
    res = S.reads_run([r1, r2], [o1, o2], fa, json=str(d / "gzp.json"), threads=6)
    return open(o1, "rb").read(), open(o2, "rb").read(), res


@pytest.mark.parametrize("chunk_mb", [None, "1"])
def test_reads_run_gz_outputs_equal_the_plain_run(dataset, plain_run, monkeypatch, capfd, chunk_mb):
    from scrubby_amd import lib as S
    d, fa, r1, r2, ids, n_pairs = dataset
    p1, p2, pres = plain_run
    monkeypatch.setenv("SCRUBBY_HIP_GZ_DEVICE", "1")
    monkeypatch.setenv("SCRUBBY_HIP_DBG_HOST", "1")
    if chunk_mb:
        monkeypatch.setenv("SCRUBBY_HIP_CHUNK_MB", chunk_mb)      # each file is ~3.3 MB: several chunks, several members
    o1, o2 = str(d / f"gzd{chunk_mb}_1.fastq.gz"), str(d / f"gzd{chunk_mb}_2.fastq.gz")
    capfd.readouterr()
    res = S.reads_run([r1, r2], [o1, o2], fa, json=str(d / f"gzd{chunk_mb}.json"), threads=6)
    err = capfd.readouterr().err
    z1, z2 = open(o1, "rb").read(), open(o2, "rb").read()
    assert gzip.decompress(z1) == p1 and gzip.decompress(z2) == p2
    assert [res[k] for k in COUNTS] == [pres[k] for k in COUNTS] and res["reads_removed"] == 2 * len(ids)
    on_device, on_host = _device_chunks(err)
    # member by member: every one is complete (CRC-32, ISIZE) and they follow each other without a gap
    n_members, rest, total = 0, z1, b""
    while rest:
        inf = zlib.decompressobj(31)
        total += inf.decompress(rest)
        assert inf.eof
        rest = inf.unused_data
        n_members += 1
    assert total == p1 and on_host == 0
    if chunk_mb is None:
        assert n_members == 1 and on_device == 2
    else:
        assert n_members >= 3 and on_device >= 2 * n_members - 1


def test_empty_output_is_one_valid_empty_member(dataset, monkeypatch, tmp_path):
    """extract mode keeps what maps; random reads do not, so nothing is written: the file is the empty member zlib leaves, as before"""
    from scrubby_amd import lib as S
    d, fa, r1, r2, ids, n_pairs = dataset
    rng = np.random.default_rng(9)
    rnd = tmp_path / "random.fastq"
    with open(rnd, "w") as f:
        for i in range(200):
            f.write(f"@rnd.{i}\n{''.join('ACGT'[k] for k in rng.integers(0, 4, 150))}\n+\n{'I' * 150}\n")
    outs = {}
    for name, env in (("off", None), ("on", "1")):
        if env:
            monkeypatch.setenv("SCRUBBY_HIP_GZ_DEVICE", env)
        o = tmp_path / f"empty_{name}.fastq.gz"
        res = S.reads_run([str(rnd)], [str(o)], fa, preset="sr", extract=True, json=str(tmp_path / f"{name}.json"))
        assert res["reads_in"] == 200 and res["reads_out"] == 0
        outs[name] = o.read_bytes()
        assert gzip.decompress(outs[name]) == b""
    assert outs["on"] == outs["off"] == zlib.compressobj(6, zlib.DEFLATED, 31).flush()


def test_switch_unset_leaves_zlibs_members(dataset, plain_run, monkeypatch):
    from scrubby_amd import lib as S
    d, fa, r1, r2, ids, n_pairs = dataset
    p1, p2, pres = plain_run
    monkeypatch.delenv("SCRUBBY_HIP_GZ_DEVICE", raising=False)
    o1, o2 = str(d / "gzu_1.fastq.gz"), str(d / "gzu_2.fastq.gz")
    res = S.reads_run([r1, r2], [o1, o2], fa, json=str(d / "gzu.json"), threads=6)
    for o, p in ((o1, p1), (o2, p2)):      # one chunk a file at the default chunk size: one member, gz_member's level 6
        c = zlib.compressobj(6, zlib.DEFLATED, 31)
        assert open(o, "rb").read() == c.compress(p) + c.flush()
    assert [res[k] for k in COUNTS] == [pres[k] for k in COUNTS]
    monkeypatch.setenv("SCRUBBY_HIP_GZ_DEVICE", "0")      # only "1" switches it on
    S.reads_run([r1, r2], [o1, o2], fa, json=str(d / "gzu.json"), threads=6)
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    assert open(o1, "rb").read() == c.compress(p1) + c.flush()


def test_kraken_run_gz_outputs_equal_the_plain_run(K, db, cfg1, tmp_path, monkeypatch, capfd):
    P, R, ref, seqs, reads, off = cfg1
    dbdir = tmp_path / "db"; dbdir.mkdir()
    db.save(dbdir)
    n_pairs = 1500
    with open(tmp_path / "p_1.fastq", "w") as f1, open(tmp_path / "p_2.fastq", "w") as f2:
        for i in range(n_pairs):
            f1.write(f"@syn.{i} 1:N:0\n{bytes(reads[(2 * i) * 150:(2 * i + 1) * 150]).decode()}\n+\n{'I' * 150}\n")
            f2.write(f"@syn.{i} 2:N:0\n{bytes(reads[(2 * i + 1) * 150:(2 * i + 2) * 150]).decode()}\n+\n{'I' * 150}\n")
    ins = [tmp_path / "p_1.fastq", tmp_path / "p_2.fastq"]
    plain = K.kraken_run(ins, [tmp_path / "q_1.fastq", tmp_path / "q_2.fastq"], dbdir, taxa=["Chordata"], taxa_direct=["9606"], workdir=tmp_path / "w0")
    monkeypatch.setenv("SCRUBBY_HIP_GZ_DEVICE", "1")
    monkeypatch.setenv("SCRUBBY_HIP_DBG_HOST", "1")
    capfd.readouterr()
    dev = K.kraken_run(ins, [tmp_path / "z_1.fastq.gz", tmp_path / "z_2.fastq.gz"], dbdir, taxa=["Chordata"], taxa_direct=["9606"], workdir=tmp_path / "w1")
    err = capfd.readouterr().err
    for m in (1, 2):
        assert gzip.decompress((tmp_path / f"z_{m}.fastq.gz").read_bytes()) == (tmp_path / f"q_{m}.fastq").read_bytes()
    assert [dev[k] for k in COUNTS] == [plain[k] for k in COUNTS] and 0 < dev["reads_out"] < 2 * n_pairs
    assert _device_chunks(err) == (2, 0)
