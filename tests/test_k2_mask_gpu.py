"""Low-complexity masking on the GPU: sh_k2_mask_device, sh_k2_build_run with mask_low_complexity, sh_k2_mask_run and
`scrubby-hip k2-mask`.

Ground truth is the brute force of the rule (tests/k2_mask_ref.py) wherever plain Python can afford it, and the library's host
mirror sh_k2_mask_host - itself pinned by the brute force in tests/test_k2_mask_cpu.py, and here again on every input the brute
force also sees - on the inputs that are too large for it.  Everything is compared byte for byte; no tolerance, no case left out.
The database tests take their expectation from the frozen oracle (k2o_scan, k2o_hash, k2o_cht_get, k2o_lca) through the helpers
of tests/test_k2_build_gpu.py, on the library as masked by the host mirror."""
import gzip
import json
import lzma
import os
import random
import subprocess

import numpy as np
import pytest

from tests import k2_mask_ref as R
from tests.test_k2_build_gpu import (E, GOLD as BUILD_GOLD, assert_no_alias, check_every_key, expected_map, fixture_parent,  # noqa: F401
                                     hashes, o_opts, open_export, read_fasta, synth_files, synth_lib, write_fasta)
from tests.test_k2_mask_cpu import PARAMS, fixture, seeded_records  # noqa: F401

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scrubby_amd", "scrubby-hip")


@pytest.fixture(scope="module")
def K():
    from scrubby_amd import lib, k2
    lib.require_gpu()
    return k2


def as_bytes(records):
    return [bytes(r) for r in records]


# ---- the kernel against the brute force -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [None, "64"])
@pytest.mark.parametrize("W,T", PARAMS)
def test_device_equals_brute_force(K, fixture, monkeypatch, W, T, tile):
    """the fixture and the seeded families, hard and soft; once more with tiles of 64 bases, so that every masked stretch of the
    inputs crosses tile borders"""
    if tile:
        monkeypatch.setenv("SCRUBBY_HIP_K2_MASK_TILE", tile)
    tl = int(tile) if tile else 4096
    recs, E_ = fixture
    e = E_["masked"][f"{W},{T}"]
    for rep in (b"x", None):
        got, st = K.mask_low_complexity(recs, W, T, rep, return_stats=True)
        assert got == R.mask_records(recs, W, T, rep)
        assert st["n_masked"] == e["n_masked"] and st["n_bases"] == E_["n_bases"]
        assert st["n_items"] == sum((len(r) + tl - 1) // tl for r in recs)
    for seed in range(100, 112):
        recs = seeded_records(seed)
        for rep in (b"x", None):
            assert K.mask_low_complexity(recs, W, T, rep) == R.mask_records(recs, W, T, rep), seed


def test_device_defaults_and_refused_parameters(K):
    from scrubby_amd import lib as S
    seq = [b"ACGT" * 3 + b"A" * 30 + b"GATTACA", b""]
    assert K.mask_low_complexity(seq, 0, 0) == K.mask_low_complexity(seq, 64, 20) == R.mask_records(seq)
    assert K.mask_low_complexity(seq, replacement=b"n") == R.mask_records(seq, replacement=b"n")
    assert K.mask_low_complexity([]) == []
    for W, T, word in ((7, 20, "window"), (65, 20, "window"), (64, -1, "threshold")):
        with pytest.raises(S.ScrubbyHipError) as ei:
            K.mask_low_complexity(seq, W, T)
        assert word in ei.value.message


# ---- the kernel against the host mirror, on inputs the brute force cannot afford --------------------------------------------------
def test_device_equals_host_on_the_build_library(K, synth_lib):
    """2 101 records, one of 2.1 Mb among 2 100 short ones"""
    records, _ = synth_lib
    recs = as_bytes(records)
    assert len(recs) == 2101 and max(len(r) for r in recs) == 2_100_000
    for W, T in PARAMS:
        got, st = K.mask_low_complexity(recs, W, T, return_stats=True)
        want, hs = K.mask_low_complexity_host(recs, W, T, return_stats=True)
        assert got == want and st["n_masked"] == hs["n_masked"] > 0
    assert K.mask_low_complexity(recs, replacement=None) == K.mask_low_complexity_host(recs, replacement=None)
    # a stretch of it under the brute force as well
    i = next(i for i, r in enumerate(recs) if 1000 <= len(r) < 1500)
    assert got[i] == R.mask_records([recs[i]], *PARAMS[-1])[0]


def test_device_equals_host_on_a_16_mb_slice_of_the_synthetic_reference(K):
    import torch
    from scrubby_amd import lib as S
    n = 16_000_000
    P = S.ref_params(0x5C2B0001, [40_000_000])
    d = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    d[n:] = ord("N")
    S.synth_ref_device(P, 12_345_678, n, d)
    ref = d[:n].cpu().numpy().tobytes()
    got, st = K.mask_low_complexity([ref], return_stats=True)
    want, hs = K.mask_low_complexity_host([ref], return_stats=True)
    print(f"16 Mb of the synthetic reference: {st}")
    assert got == want and st["n_masked"] == hs["n_masked"]
    assert 0.001 < st["n_masked"] / n < 0.5          # its satellite families are low-complexity, the rest is not


# ---- position independence ------------------------------------------------------------------------------------------------------
def test_position_independence(K, fixture):
    """the same record alone, as record 1 000 of a batch, and at every byte offset modulo 8; a record of one tile plus one base"""
    recs, _ = fixture
    rng = random.Random(5)
    probe = max(recs[:24], key=len)          # the longest of the family mixes
    assert len(probe) > 1500
    alone = K.mask_low_complexity([probe])[0]
    assert alone == R.mask_records([probe])[0]
    for shift in range(8):
        filler = [b"ACGTTGCA" * 3 + b"A" * shift]          # 24 + shift bases in front: the record starts at every offset modulo 8
        got = K.mask_low_complexity(filler + [probe])
        assert got[1] == alone, shift
    batch = [("".join(rng.choice("ACGT") for _ in range(rng.randrange(0, 90)))).encode() for _ in range(1000)] + [probe, b"T" * 50]
    got = K.mask_low_complexity(batch)
    assert got[1000] == alone and got[1001] == b"x" * 50 and got[:1000] == R.mask_records(batch[:1000])
    one_more = ("".join(rng.choice("ACGT") for _ in range(4060)) + "A" * 37).encode()          # the stretch ends in the second tile
    assert len(one_more) == 4097
    assert K.mask_low_complexity([one_more]) == R.mask_records([one_more])


# ---- the build run --------------------------------------------------------------------------------------------------------------
def table_get(oracle, cells, value_bits, keys):
    t = oracle.K2Table(cells, np.zeros(1, np.uint32), value_bits)
    return np.array([t.get(int(k)) for k in keys], dtype=np.uint32)


def test_masked_build(K, oracle, E, synth_lib, fixture_parent, tmp_path):
    """(a) the database does not depend on chunk_bytes; (b) it holds every minimizer of the masked library under the LCA of its
    records' taxa; (c) the minimizers that only the unmasked library has are absent, and there are such"""
    records, taxa = synth_lib
    fna, mp = synth_files(tmp_path, synth_lib, E)
    vb = E["value_bits"]
    o = o_opts(oracle, vb)
    masked, hs = K.mask_low_complexity_host(as_bytes(records), return_stats=True)
    masked = [np.frombuffer(m, dtype=np.uint8) for m in masked]
    keys, vals = expected_map(oracle, o, masked, taxa, fixture_parent)
    keys0, _ = expected_map(oracle, o, records, taxa, fixture_parent)
    gone = np.setdiff1d(keys0, keys)
    print(f"{len(keys0)} distinct minimizers unmasked, {len(keys)} masked, {len(gone)} only unmasked")
    assert len(gone) >= 0.01 * len(keys0)
    n_masked_taxon = sum(int((m == ord("x")).sum()) for m, t in zip(masked, taxa) if t)
    big = 2_100_000
    runs = {"whole": 0, "cut12": big // 13, "cut97": big // 99}
    res, tables = {}, {}
    for name, chunk in runs.items():
        res[name] = K.build_database([fna], tmp_path / name, taxonomy_dir=BUILD_GOLD, seqid2taxid=mp, chunk_bytes=chunk, mask=True)
        tables[name] = open_export(K, tmp_path / name)
        print(name, res[name])
    assert res["whole"]["n_cuts"] == 0 and res["cut12"]["n_cuts"] >= 12 and res["cut97"]["n_cuts"] >= 97
    cap = res["whole"]["capacity"]
    assert_no_alias(hashes(oracle, keys), cap, vb)
    union = np.union1d(keys0, keys)
    ref_vals = table_get(oracle, tables["whole"][0][0], vb, union)
    for name in runs:
        r = res[name]
        assert r["n_masked_bases"] == n_masked_taxon and r["n_bases"] == res["whole"]["n_bases"]
        assert (r["capacity"], r["size"], r["n_sampled"]) == (cap, len(keys), res["whole"]["n_sampled"])
        (cells, _, _), info = tables[name]
        assert info["size"] == len(keys) and int((cells != 0).sum()) == len(keys)
        assert np.array_equal(table_get(oracle, cells, vb, union), ref_vals), name          # (a) per key over the union
        check_every_key(oracle, cells, vb, keys, vals)                                      # (b)
        assert not table_get(oracle, cells, vb, gone).any()                                 # (c)
    # another window and threshold go through as well
    r16 = K.build_database([fna], tmp_path / "w16", taxonomy_dir=BUILD_GOLD, seqid2taxid=mp, chunk_bytes=300_000, mask=True, mask_window=16, mask_threshold=12)
    m16 = K.mask_low_complexity_host(as_bytes(records), 16, 12)
    assert r16["n_masked_bases"] == sum(m.count(b"x") for m, t in zip(m16, taxa) if t)
    k16, v16 = expected_map(oracle, o, [np.frombuffer(m, dtype=np.uint8) for m in m16], taxa, fixture_parent)
    (cells, _, _), info = open_export(K, tmp_path / "w16")
    assert info["size"] == len(k16)
    check_every_key(oracle, cells, vb, k16, v16)


def test_flag_off_writes_what_it_wrote(K, oracle, E, synth_lib, fixture_parent, tmp_path):
    """(d) without the flag: the table of the unmasked library, as before; and the masking options alone are refused"""
    from scrubby_amd import lib as S
    records, taxa = synth_lib
    fna, mp = synth_files(tmp_path, synth_lib, E)
    vb = E["value_bits"]
    keys0, vals0 = expected_map(oracle, o_opts(oracle, vb), records, taxa, fixture_parent)
    off = K.build_database([fna], tmp_path / "off", taxonomy_dir=BUILD_GOLD, seqid2taxid=mp, chunk_bytes=300_000)
    on = K.build_database([fna], tmp_path / "on", taxonomy_dir=BUILD_GOLD, seqid2taxid=mp, chunk_bytes=300_000, mask=True)
    assert off["n_masked_bases"] == 0 and off["s_mask"] == 0 and off["size"] == len(keys0) and on["size"] < off["size"]
    for name in ("opts.k2d", "taxo.k2d"):
        assert open(tmp_path / "off" / name, "rb").read() == open(tmp_path / "on" / name, "rb").read(), name
    (cells, _, _), info = open_export(K, tmp_path / "off")
    check_every_key(oracle, cells, vb, keys0, vals0)
    assert int((cells != 0).sum()) == len(keys0)
    with pytest.raises(S.ScrubbyHipError) as ei:
        K.build_database([fna], tmp_path / "bad", taxonomy_dir=BUILD_GOLD, seqid2taxid=mp, mask_window=32)
    assert "--mask-low-complexity" in ei.value.message


# ---- the point of it all --------------------------------------------------------------------------------------------------------
def test_masked_database_keeps_the_reads_that_only_share_low_complexity(K, oracle, tmp_path):
    """A single-taxon database from a reference with poly-A and microsatellite stretches.  Reads of random sequence around such a
    stretch share nothing else with the reference; reads drawn from its ordinary sequence are the host's.  Built unmasked,
    `-T 9606` removes both kinds; built masked, the first kind stays and the second is still removed.  Every call equals
    K2Table.classify of the frozen oracle on the exported table."""
    rng = np.random.default_rng(20261016)
    rs = lambda n: bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, n))
    stretches = [b"A" * 90, b"CA" * 45, b"T" * 90, b"GAA" * 30, b"AC" * 45, b"TTAGGG" * 15]
    ref = b"".join(rs(6000) + s for s in stretches * 3) + rs(6000)
    write_fasta(tmp_path / "host.fa", [("chrS synthetic with simple repeats", ref)], width=60)
    reads, kind = [], []
    for i in range(240):          # two different stretches each: two hit groups, Kraken 2's default minimum
        s1, s2 = stretches[i % len(stretches)], stretches[(i + 1) % len(stretches)]
        reads.append(rs(10) + s1[:62] + rs(6) + s2[:62] + rs(10)); kind.append("lc")
    for i in range(240):
        p = int(rng.integers(0, 5800)) + 6090 * int(rng.integers(0, 18))          # inside one of the random blocks
        reads.append(ref[p: p + 150]); kind.append("host")
    order = rng.permutation(len(reads))
    reads, kind = [reads[i] for i in order], [kind[i] for i in order]
    with open(tmp_path / "in.fastq", "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@r{i}\n{r.decode()}\n+\n{'I' * len(r)}\n")
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    o = o_opts(oracle, 2)
    lc = {f"r{i}" for i, k in enumerate(kind) if k == "lc"}
    host = {f"r{i}" for i, k in enumerate(kind) if k == "host"}
    for name, mask in (("plain", False), ("masked", True)):
        res = K.build_database([tmp_path / "host.fa"], tmp_path / name, taxid=9606, name="Homo sapiens", mask=mask)
        (cells, parent, ext), info = open_export(K, tmp_path / name)
        c = oracle.K2Table(cells, parent, 2).classify(o, bases, off, threads=4)
        d = K.K2Db.open(tmp_path / name)
        g, _ = d.classify(bases, off)
        d.close()
        for field in ("call", "total_kmers", "hit_groups"):
            assert np.array_equal(g[field], c[field]), (name, field)
        K.kraken_run([tmp_path / "in.fastq"], [tmp_path / f"out_{name}.fastq"], tmp_path / name, taxa=["9606"], workdir=tmp_path / f"w_{name}")
        kept = {ln[1:].strip() for ln in open(tmp_path / f"out_{name}.fastq") if ln.startswith("@r")}
        assert kept == {f"r{i}" for i in np.flatnonzero(c["call"] != 2)}
        print(name, res["n_masked_bases"], "masked bases;", len(kept & lc), "low-complexity reads and", len(kept & host), "host reads kept")
        if mask:
            assert kept == lc and res["n_masked_bases"] >= sum(len(s) for s in stretches) * 3
        else:
            assert kept == set() and res["n_masked_bases"] == 0


# ---- scrubby-hip k2-mask --------------------------------------------------------------------------------------------------------
def test_k2_mask_cli(K, fixture, tmp_path):
    recs, E_ = fixture
    heads = [r["header"] for r in E_["records"]]
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k2_mask", "library.fa")
    want = K.mask_low_complexity(recs)
    p = subprocess.run([EXE, "k2-mask", "-i", src, "-o", str(tmp_path / "m.fa")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    j = json.loads(p.stdout.strip().splitlines()[-1])
    assert (j["records"], j["bases"], j["masked_bases"], j["cuts"]) == (len(recs), E_["n_bases"], E_["masked"]["64,20"]["n_masked"], 0)
    out = read_fasta(tmp_path / "m.fa")
    assert [h for h, _ in out] == heads and [s for _, s in out] == want
    lines = open(tmp_path / "m.fa", "rb").read().split(b"\n")
    assert max(len(ln) for ln in lines if not ln.startswith(b">")) == 60
    # gzip in, xz out, soft, another window, one line per record; cut many times by a small chunk
    with gzip.open(tmp_path / "in.fa.gz", "wb") as f:
        f.write(open(src, "rb").read())
    soft = K.mask_low_complexity(recs, 32, 20, None)
    for name, extra in (("uncut", []), ("cut", ["--chunk-bytes", "700"])):
        p = subprocess.run([EXE, "k2-mask", "-i", str(tmp_path / "in.fa.gz"), "-o", str(tmp_path / f"{name}.fa.xz"), "--soft", "-W", "32", "--line-width", "0"] + extra,
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        j = json.loads(p.stdout.strip().splitlines()[-1])
        assert j["masked_bases"] == E_["masked"]["32,20"]["n_masked"] and (j["cuts"] >= 5) == bool(extra)
        text = lzma.open(tmp_path / f"{name}.fa.xz").read()
        assert text == b"".join(b">" + h.encode() + b"\n" + (s + b"\n" if s else b"") for h, s in zip(heads, soft))
        assert [s.upper() for s in soft] == [r.upper() for r in recs]
    # the library call on a file: hard masking with another byte, cut, wrapped at 50
    r = K.mask_file(src, tmp_path / "lib.fa", replacement=b"n", line_width=50, chunk_bytes=1500)
    assert r["n_masked_bases"] == E_["masked"]["64,20"]["n_masked"] and r["n_cuts"] >= 5 and r["n_records"] == len(recs)
    out = read_fasta(tmp_path / "lib.fa")
    assert [h for h, _ in out] == heads and [s for _, s in out] == K.mask_low_complexity(recs, replacement=b"n")
    p = subprocess.run([EXE, "k2-mask", "-i", src, "-o", str(tmp_path / "bad.fa"), "-W", "100"], capture_output=True, text=True)
    assert p.returncode == 1 and "window" in p.stderr
    p = subprocess.run([EXE], capture_output=True, text=True)
    assert "k2-mask" in p.stderr and "--mask-low-complexity" in p.stderr
