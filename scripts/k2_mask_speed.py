"""Speed of low-complexity masking before the Kraken arm's database build (DESIGN.md §7 "Low-complexity masking").

mask      sh_k2_mask_device on (i) --mask-bases of the synthetic CHM13v2-sized reference bench.py uses and (ii) as many bases
          of a worst case in which every step is low-complexity (a 5-base unit repeated, one substitution per 485 bases, cut into
          1 Mb records); wall time of the whole call, synchronisation included, on a fresh copy of the input each time; median,
          minimum and maximum of --launches runs, and the device time the call itself reports.  (i) is also run with other tile
          lengths (SCRUBBY_HIP_K2_MASK_TILE) to record the choice of 4096.
build     `scrubby-hip k2-build --taxid 9606` on a FASTA of the whole synthetic reference (3.1 Gb), three ways, alternating,
          --rounds times: the parent commit's binary (--parent-exe, optional), this tree without the flag, this tree with
          --mask-low-complexity.  The seconds per phase each run prints, and for the masked run the time in the mask calls.

    python scripts/k2_mask_speed.py [--launches 7] [--rounds 2] [--small] [--no-build] [--parent-exe PATH] [--work DIR] [--out profiles/k2_mask.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B  # noqa: E402
from scrubby_amd import k2 as K  # noqa: E402
from scrubby_amd import lib as S  # noqa: E402
import ctypes as C  # noqa: E402


def summary(xs):
    return {"median_s": round(statistics.median(xs), 5), "min_s": round(min(xs), 5), "max_s": round(max(xs), 5), "runs": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--mask-bases", type=int, default=1_000_000_000)
    ap.add_argument("--small", action="store_true", help="a rehearsal: 8 Mb, a 5 x 1 Mb reference")
    ap.add_argument("--no-build", action="store_true")
    ap.add_argument("--parent-exe")
    ap.add_argument("--work", default="/tmp/k2_mask_speed")
    ap.add_argument("--out")
    a = ap.parse_args()
    S.require_gpu()
    L = S.load()
    dev = torch.device("cuda:0")
    n = 8_000_000 if a.small else a.mask_bases
    rec = 1_000_000
    d_off = torch.arange(0, n + 1, rec, dtype=torch.int64, device=dev)
    n_rec = len(d_off) - 1
    d_work = torch.empty(n + 64, dtype=torch.uint8, device=dev)

    def timed(d_src, runs):
        ts, st = [], K.K2MaskStats()
        for i in range(runs + 1):          # one warm-up
            d_work.copy_(d_src)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            S.check(L.sh_k2_mask_device(C.c_void_p(d_work.data_ptr()), C.c_void_p(d_off.data_ptr()), C.c_uint64(n_rec), 0, 0, ord("x"), None, C.byref(st)))
            ts.append(time.perf_counter() - t0)
        r = summary(ts[1:])
        r.update(device_ms=round(st.ms, 3), n_masked=st.n_masked, n_items=st.n_items, masked_pct=round(100.0 * st.n_masked / n, 3),
                 s_per_gb=round(r["median_s"] * 1e9 / n, 4))
        return r

    res = {"workload": {"bases": n, "records": n_rec, "record_len": rec}, "launches": a.launches}
    P = S.ref_params(B.REF_SEED, [n])
    d_ref = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    S.synth_ref_device(P, 0, n, d_ref)
    d_ref[n:] = ord("N")
    res["i_synthetic_reference"] = timed(d_ref, a.launches)
    res["tile_sweep"] = {}
    for tile in (1024, 2048, 4096, 8192, 16384):
        os.environ["SCRUBBY_HIP_K2_MASK_TILE"] = str(tile)
        res["tile_sweep"][str(tile)] = timed(d_ref, a.launches)
    del os.environ["SCRUBBY_HIP_K2_MASK_TILE"]
    unit = np.frombuffer(b"ACGTT" * 97, dtype=np.uint8).copy()
    unit[41] = ord("G")
    worst = np.resize(unit, n + 64)
    worst[n:] = ord("N")
    d_ref.copy_(torch.from_numpy(worst).to(dev))
    res["ii_every_step_low_complexity"] = timed(d_ref, a.launches)
    del d_ref, d_work
    torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)

    if not a.no_build:
        contigs = [1_000_000] * 5 if a.small else B.CHM13_CONTIGS
        P = S.ref_params(B.REF_SEED, contigs)
        G = P.genome_len
        os.makedirs(a.work, exist_ok=True)
        fa = os.path.join(a.work, "ref.fa")
        d = torch.empty(G + 64, dtype=torch.uint8, device=dev)
        S.synth_ref_device(P, 0, G, d)
        h = d[:G].cpu().numpy()
        del d
        torch.cuda.empty_cache()
        with open(fa, "wb") as f:
            for i in range(len(contigs)):
                f.write(b">ctg%d synthetic\n" % i)
                h[P.contig_start[i]:P.contig_start[i + 1]].tofile(f)
                f.write(b"\n")
        del h
        ways = []
        if a.parent_exe:
            ways.append(("parent", a.parent_exe, []))
        exe = os.path.join(ROOT, "scrubby_amd", "scrubby-hip")
        ways += [("flag_off", exe, []), ("flag_on", exe, ["--mask-low-complexity"])]
        runs = {w[0]: [] for w in ways}
        for rnd in range(a.rounds):
            for name, x, extra in ways:
                t0 = time.time()
                p = subprocess.run([x, "k2-build", "-i", fa, "-o", os.path.join(a.work, "db_" + name), "--taxid", "9606", "--name", "Homo sapiens"] + extra,
                                   capture_output=True, text=True)
                wall = time.time() - t0
                for f in ("hash.k2d", "opts.k2d", "taxo.k2d"):          # 5 GB a table: gone before the next run
                    try:
                        os.remove(os.path.join(a.work, "db_" + name, f))
                    except OSError:
                        pass
                if p.returncode != 0:
                    runs[name].append({"error": p.stderr[-500:]})
                    continue
                j = json.loads(p.stdout.strip().splitlines()[-1])
                j["wall_s"] = round(wall, 2)
                j["gpu_s_both_passes"] = round(j["s_fill"] + j["s_estimate"] - j["s_read"], 3)
                runs[name].append(j)
                print(name, json.dumps(j), flush=True)
        res["build"] = {"fasta_bytes": os.path.getsize(fa), "rounds": a.rounds, "runs": runs,
                        "s_total_median": {k: round(statistics.median([r["s_total"] for r in v if "s_total" in r]), 3) for k, v in runs.items() if any("s_total" in r for r in v)}}
        os.remove(fa)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
