"""BGZF inflate on the device (sh_inflate.hip) on the e2e bench's FASTQ (scripts/deflate_speed.py fastq_bytes), --mib MiB of it
bgzip-shaped by tests/bgzf_util.py (members of 65 280 bytes, zlib level 6).  Three parts, one JSON line each, also written to
--out-dir as gunzip_device_{kernel,index,e2e}.json:

  kernel  the compressed bytes resident in HBM, k_inflate_member between two events: GB/s of output over all members, and the time for
          33, 4 096 and 32 768 members in flight (does the rate scale with resident waves?); where the file has fewer members than that,
          they are listed again, each listing decoded into a place of its own
  index   sh_index_build_fasta on a bgzipped synthetic reference of --ref-mb Mb, SCRUBBY_HIP_GUNZIP_DEVICE off against on, same process,
          after one warm-up of each
  e2e     sh_reads_run on the BGZF FASTQ (single-end) against that reference, switch off against on

The switch-off run is the comparison: with the switch unset the code is the parent's.

    python scripts/inflate_speed.py --mib 1024 --ref-mb 3100 --out-dir profiles
"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.deflate_speed import fastq_bytes      # noqa: E402
from tests import bgzf_util as B                   # noqa: E402


def bgzf_parallel(data, threads=16):
    """bgzf_util.bgzf over slabs of 256 members on a thread pool (zlib releases the interpreter lock)"""
    slab = 256 * B.BLOCK
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda o: B.bgzf(bytes(data[o:o + slab]), eof=False), range(0, len(data), slab)))
    return b"".join(parts) + B.EOF


def emit(a, name, rec):
    print(json.dumps(rec), flush=True)
    if a.out_dir:
        with open(os.path.join(a.out_dir, f"gunzip_device_{name}.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


def part_kernel(a, S, text, file_bytes):
    import torch
    members, used, stopped = S.bgzf_scan(file_bytes)
    assert used == len(file_bytes) and stopped == 0
    n_out = sum(m.out_len for m in members)
    d_in = torch.frombuffer(bytearray(file_bytes), dtype=torch.uint8).cuda()
    d_out = torch.empty(n_out + 64, dtype=torch.uint8, device="cuda")
    inf = S.Inflater(len(file_bytes), n_out, len(members))
    runs = [inf.inflate_members_device(d_in, members, d_out) for _ in range(a.steps + 1)]      # the first run is the warm-up
    assert d_out[:1 << 20].cpu().numpy().tobytes() == bytes(text[:1 << 20]) and d_out[n_out - 4096:n_out].cpu().numpy().tobytes() == bytes(text[-4096:])
    ms = sorted(r["ms"] for r in runs[1:])[a.steps // 2]
    st = runs[-1]
    inf.close()
    in_flight = {}
    for k in (33, 4096, 32768):
        # the resident members listed as often as it takes: each listing is decoded again, into a place of its own
        sub = (members * -(-k // len(members)))[:k]
        k_out = sum(m.out_len for m in sub)
        if k_out > n_out:
            d_out = None
            d_out = torch.empty(k_out + 64, dtype=torch.uint8, device="cuda")
        inf_k = S.Inflater(len(file_bytes), k_out, k)
        rs = [inf_k.inflate_members_device(d_in, sub, d_out) for _ in range(a.steps + 1)]
        inf_k.close()
        m = sorted(r["ms"] for r in rs[1:])[a.steps // 2]
        in_flight[str(k)] = {"ms": round(m, 3), "out_bytes": rs[-1]["out_bytes"], "output_GB_per_s": round(rs[-1]["out_bytes"] / m / 1e6, 2)}
    emit(a, "kernel", {
        "workload": f"k_inflate_member on {a.mib} MiB of the e2e bench's FASTQ as BGZF (members of {B.BLOCK} bytes, zlib level 6), resident in HBM",
        "device": torch.cuda.get_device_name(0), "n_members": st["n_members"], "in_bytes": st["in_bytes"], "out_bytes": st["out_bytes"],
        "dynamic_blocks": st["n_dynamic_blocks"], "ms": round(ms, 2), "ms_runs": [round(r["ms"], 2) for r in runs[1:]],
        "output_GB_per_s": round(st["out_bytes"] / ms / 1e6, 2), "members_in_flight": in_flight})


def timed(fn, env):
    """wall seconds of fn() with SCRUBBY_HIP_GUNZIP_DEVICE set to env (None: unset)"""
    if env is None:
        os.environ.pop("SCRUBBY_HIP_GUNZIP_DEVICE", None)
    else:
        os.environ["SCRUBBY_HIP_GUNZIP_DEVICE"] = env
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def part_index_and_e2e(a, S, text, file_bytes, work):
    import torch
    contigs = [a.ref_mb * 1_000_000 // 4] * 4
    P = S.ref_params(0x5C2B0001, contigs)
    d_ref = torch.empty(P.genome_len + 64, dtype=torch.uint8, device="cuda")
    S.synth_ref_device(P, 0, P.genome_len, d_ref)
    h_ref = d_ref[:P.genome_len].cpu().numpy()
    del d_ref
    fasta = b"".join(b">ctg%d synthetic\n" % i + h_ref[P.contig_start[i]:P.contig_start[i + 1]].tobytes() + b"\n" for i in range(len(contigs)))
    fa = os.path.join(work, "ref.fa.gz")
    with open(fa, "wb") as f:
        f.write(bgzf_parallel(fasta))
    opts = S.preset("sr")
    rec = {"workload": f"sh_index_build_fasta on a bgzipped synthetic reference of {a.ref_mb} Mb ({os.path.getsize(fa)} bytes compressed)",
           "device": torch.cuda.get_device_name(0), "runs": {}}
    infos = {}
    for name, env in (("switch_off", None), ("switch_on", "1")):
        timed(lambda: S.Index.build_fasta(fa, opts).close(), env)      # warm-up
        secs = []
        for _ in range(a.steps):
            t, idx = timed(lambda: S.Index.build_fasta(fa, opts), env)
            infos[name] = {k: v for k, v in idx.info().items() if k != "build_ms"}
            idx.close()
            secs.append(t)
        rec["runs"][name] = {"seconds": [round(t, 3) for t in secs], "median_s": round(sorted(secs)[len(secs) // 2], 3)}
    rec["same_index"] = infos["switch_off"] == infos["switch_on"]
    rec["speedup"] = round(rec["runs"]["switch_off"]["median_s"] / rec["runs"]["switch_on"]["median_s"], 2)
    emit(a, "index", rec)

    fq = os.path.join(work, "reads.fastq.gz")
    with open(fq, "wb") as f:
        f.write(file_bytes)
    n_reads = bytes(text).count(b"\n") // 4
    rec = {"workload": f"sh_reads_run, single-end, {n_reads} reads of the e2e bench's FASTQ as BGZF ({len(file_bytes)} bytes) against that reference, plain output",
           "device": torch.cuda.get_device_name(0), "runs": {}}
    outs = {}
    for name, env in (("switch_off", None), ("switch_on", "1")):
        out = os.path.join(work, f"out_{name}.fastq")
        run = lambda: S.reads_run([fq], [out], fa, preset="sr", json=os.path.join(work, "r.json"), threads=16)      # noqa: E731
        timed(run, env)      # warm-up: the index of this reference is built and kept
        secs = []
        for _ in range(a.steps):
            t, res = timed(run, env)
            secs.append(t)
        outs[name] = (res["reads_in"], res["reads_out"], os.path.getsize(out))
        med = sorted(secs)[len(secs) // 2]
        rec["runs"][name] = {"seconds": [round(t, 3) for t in secs], "median_s": round(med, 3), "M_reads_per_s": round(n_reads / med / 1e6, 2)}
    rec["same_counts_and_output_size"] = outs["switch_off"] == outs["switch_on"]
    rec["speedup"] = round(rec["runs"]["switch_off"]["median_s"] / rec["runs"]["switch_on"]["median_s"], 2)
    emit(a, "e2e", rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--ref-mb", type=int, default=3100)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--parts", default="kernel,index,e2e")
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    from scrubby_amd import lib as S
    S.require_gpu()
    text = fastq_bytes(S, a.mib << 20, "cuda")
    text = text[:len(text) - len(text) % 327]      # whole records: 23 bytes of header, 150 bases, `\n+\n`, 150 qualities, `\n`
    file_bytes = bgzf_parallel(text)
    parts = a.parts.split(",")
    if "kernel" in parts:
        part_kernel(a, S, text, file_bytes)
    if "index" in parts or "e2e" in parts:
        with tempfile.TemporaryDirectory(prefix="scrubby_gunzip_") as work:
            part_index_and_e2e(a, S, text, file_bytes, work)


if __name__ == "__main__":
    main()
