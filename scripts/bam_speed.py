"""`scrubby alignment` on BAM: the device path (sh_bam.hip behind SCRUBBY_HIP_GUNZIP_DEVICE=1) against the host path (zlib and
sh_bam_filter_host on one thread), on two files written by tests/bam_util.py and bgzip-shaped by tests/bgzf_util.py:

  short   reads of 150 bases, `150M` or a soft clip and a match, --mib MiB inflated
  long    reads of 10 .. 100 kb with CIGARs of thousands of ops, --long-mib MiB inflated

For each, one JSON line per part, all of them also in --out-dir/bam_device.json:

  stages  the file's members inflated into HBM (sh_inflate_members_device), then sh_bam_filter_device on the whole record stream:
          ms and GB/s of the inflate, of k_bam_probe, of the chain (k_bam_chain and the host's waits) and of k_bam_filter with the scan;
          the median of --steps calls after one warm-up
  e2e     sh_alignment_run on the file with a small FASTQ, the switch off against on, each in a process of its own after a warm-up
          on a small file; the switch-off run is the comparison

Every part runs in a child process under a time limit of its own; the first one that fails ends the script.

    python scripts/bam_speed.py --mib 256 --long-mib 128 --out-dir profiles
"""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.inflate_speed import bgzf_parallel      # noqa: E402
from tests import bam_util as B                      # noqa: E402


QUAL = bytes(i % 41 for i in range(256))                                              # random bytes -> Phred 0..40
SEQ = bytes((1, 2, 4, 8)[i & 3] << 4 | (1, 2, 4, 8)[i >> 2 & 3] for i in range(256))      # random bytes -> two of A C G T


def bases(rng, l_seq):
    """random bases and qualities, so that the file compresses as a BAM does and not as a run of one byte"""
    return dict(seq=rng.randbytes((l_seq + 1) // 2).translate(SEQ), qual=rng.randbytes(l_seq).translate(QUAL))


def short_records(mib):
    rng = random.Random(3)
    out, size, i = [], 0, 0
    while size < mib << 20:
        k = i % 40
        rec = B.encode(B.Rec(name=b"SRR0.%d" % i, cigar=((B.M, 150),) if k > 8 else ((B.S, 10 * k + 5), (B.M, 145 - 10 * k)), mapq=i % 61, flag=4 if i % 29 == 0 else 16 * (i & 1),
                             aux=(("NM", "i", i % 7), ("AS", "i", 290 - k)), **bases(rng, 150)))
        out.append(rec); size += len(rec); i += 1
    return B.header(3) + b"".join(out), i


def long_records(mib):
    rng = random.Random(5)
    out, size, i = [], 0, 0
    while size < mib << 20:
        n_ops = rng.randrange(500, 6000)
        per = rng.randrange(10000, 100000) // n_ops + 1
        cigar = tuple((B.M, per) if j % 2 == 0 else ((B.I, 2) if j % 4 == 1 else (B.D, 3)) for j in range(n_ops))
        rec = B.encode(B.Rec(name=b"ont.%d" % i, cigar=cigar, mapq=i % 61, **bases(rng, sum(n for op, n in cigar if op in B.QUERY_OPS))))
        out.append(rec); size += len(rec); i += 1
    return B.header(3) + b"".join(out), i


def part_stages(a):
    import torch
    from scrubby_amd import lib as S
    data = open(a.file, "rb").read()
    members, used, stopped = S.bgzf_scan(data)
    assert used == len(data) and stopped == 0
    n_out = sum(m.out_len for m in members)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    d_text = torch.empty(n_out + 64, dtype=torch.uint8, device="cuda")
    inf = S.Inflater(len(data), n_out, len(members))
    head = None
    runs = []
    scanner = S.BamScanner(n_out)
    d_names = torch.empty(S.bam_names_bound(n_out), dtype=torch.uint8, device="cuda")
    for _ in range(a.steps + 1):
        ist = inf.inflate_members_device(d_in, members, d_text)
        if head is None:
            head = S.bam_header(d_text[:1 << 16].cpu().numpy().tobytes())
            assert head[0] == 0
        names_len, nxt, st = scanner.filter_device(d_text, n_out, head[1], d_names, entry=head[2], last=True, min_len=100, min_cov=2.0, min_mapq=20)
        assert nxt == n_out
        runs.append(dict(ms_inflate=ist["ms"], **st))
    med = {k: sorted(r[k] for r in runs[1:])[(len(runs) - 1) // 2] for k in ("ms_inflate", "ms_probe", "ms_chain", "ms_filter", "ms")}
    gbs = {k.replace("ms", "gbs"): round(n_out / 1e6 / v, 2) for k, v in med.items() if v > 0}
    last = runs[-1]
    print(json.dumps(dict(part="stages", file=os.path.basename(a.file), compressed_bytes=len(data), inflated_bytes=n_out, n_members=len(members),
                          **{k: last[k] for k in ("n_records", "n_selected", "n_segments", "n_plausible", "n_fallback_segments", "name_bytes")},
                          **{k: round(v, 3) for k, v in med.items()}, **gbs, chain_share=round(med["ms_chain"] / med["ms"], 3))), flush=True)


def part_e2e(a):
    from scrubby_amd import lib as S
    S.alignment_run([a.fastq], [a.fastq + ".warm"], a.warm, min_len=100, min_cov=2.0, min_mapq=20)
    t0 = time.perf_counter()
    res = S.alignment_run([a.fastq], [a.fastq + ".out"], a.file, min_len=100, min_cov=2.0, min_mapq=20)
    dt = time.perf_counter() - t0
    print(json.dumps(dict(part="e2e", file=os.path.basename(a.file), switch=os.environ.get("SCRUBBY_HIP_GUNZIP_DEVICE", ""), seconds=round(dt, 3),
                          n_depleted_ids=res["n_depleted_ids"], inflated_gbs=round(a.inflated / 1e9 / dt, 3))), flush=True)


def child(args, env_switch, limit):
    env = {k: v for k, v in os.environ.items() if k != "SCRUBBY_HIP_GUNZIP_DEVICE"}
    if env_switch:
        env["SCRUBBY_HIP_GUNZIP_DEVICE"] = env_switch
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"part {args} failed with {p.returncode}: nothing more is started")
    line = [l for l in p.stdout.split("\n") if l.startswith("{")][-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--long-mib", type=int, default=128)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds a part may take")
    ap.add_argument("--part", default=None)
    ap.add_argument("--file"); ap.add_argument("--fastq"); ap.add_argument("--warm"); ap.add_argument("--inflated", type=int, default=0)
    a = ap.parse_args()
    if a.part == "stages":
        return part_stages(a)
    if a.part == "e2e":
        return part_e2e(a)
    results = []
    with tempfile.TemporaryDirectory() as d:
        fq = os.path.join(d, "r.fq")
        with open(fq, "w") as f:
            f.write("".join(f"@SRR0.{i}\nACGT\n+\nIIII\n" for i in range(0, 20000, 2)))
        warm = os.path.join(d, "warm.bam")
        with open(warm, "wb") as f:
            f.write(B.bam_file(3, [B.aligned(b"w%d" % i) for i in range(100)]))
        for kind, make, mib in (("short", short_records, a.mib), ("long", long_records, a.long_mib)):
            text, n_rec = make(mib)
            path = os.path.join(d, kind + ".bam")
            with open(path, "wb") as f:
                f.write(bgzf_parallel(text))
            results.append(dict(kind=kind, n_written=n_rec, **child(["--part", "stages", "--file", path, "--steps", str(a.steps)], None, a.limit)))
            for switch in (None, "1"):
                results.append(dict(kind=kind, **child(["--part", "e2e", "--file", path, "--fastq", fq, "--warm", warm, "--inflated", str(len(text))], switch, a.limit)))
    if a.out_dir:
        with open(os.path.join(a.out_dir, "bam_device.json"), "w") as f:
            json.dump(dict(note="one box, these sizes", results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
