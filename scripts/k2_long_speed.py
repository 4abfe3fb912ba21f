"""The Kraken arm on long reads: the lane route (k_k2_classify, one lane per unit) against the wave route (k_k2_classify_wave,
one wave per unit of at least opts.long_unit_bases bases), on the synthetic table of scripts/k2_hits_speed.py (2e9 cells, the
CHM13-sized synthetic reference under Homo sapiens plus filler keys).

Workloads, resident in HBM:
  a   200 000 long reads with the length law of bench.py --workload ont (syn_long_len, sh_synth_long_reads_device)
  b   200 000 reads of 10 000 bases each (the lane route at its best: no imbalance)
  c   the configs[4] stand-in of scripts/k2_options_speed.py, 2x150 bp pairs (no long unit)
Each workload runs the plain and the hit-list forms with long_unit_bases = -1 (never), 1024 ... 32768: one warm-up launch, then
--launches launches; the median, the smallest and the largest sh_k2_stats.ms_classify are recorded (and ms_long, the wave
kernel's share).  A build without the option (an older library) runs the one mode it has, as the baseline for "-1 is that speed".
Prints one JSON object; --out writes it too.

    python scripts/k2_long_speed.py [--launches 7] [--small] [--workloads a,b,c] [--out profiles/k2_long.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B  # noqa: E402
from scrubby_amd import k2 as K  # noqa: E402
from scrubby_amd import lib as S  # noqa: E402

THRESHOLDS = [-1, 1024, 2048, 4096, 8192, 16384, 32768]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="5 x 1 Mb reference, 12 M cells, a tenth of the reads (a rehearsal)")
    ap.add_argument("--workloads", default="a,b,c")
    ap.add_argument("--out")
    a = ap.parse_args()
    S.require_gpu()
    dev = torch.device("cuda:0")
    contigs = [1_000_000] * 5 if a.small else B.CHM13_CONTIGS
    cells = 12_000_017 if a.small else 2_000_000_000
    n_long = 20_000 if a.small else 200_000
    n_short = 200_000 if a.small else 40_000_000
    P = S.ref_params(B.REF_SEED, contigs)
    G = P.genome_len
    t0 = time.time()
    parents, externals, names, ranks, ids = B.k2_taxonomy(2_000 if a.small else 50_000, 0x5C2B0030)
    db = K.K2Db.create(K.default_opts(), cells, parents, externals, names, ranks)
    d_ref = torch.empty(G + 64, dtype=torch.uint8, device=dev)
    S.synth_ref_device(P, 0, G, d_ref)
    db.insert_sequence_device(d_ref, G, ids["Homo sapiens"])
    del d_ref
    torch.cuda.empty_cache()
    db.insert_random(0x5C2B0031, max(int(0.70 * cells) - db.info()["size"], 0), ids["Bacteria"], len(parents) - 1)
    torch.cuda.synchronize()
    has_route = hasattr(db.opts(), "long_unit_bases")
    out = {"table": f"{cells} cells, k=35 l=31, confidence 0, minimum-hit-groups 2", "launches": a.launches, "setup_s": round(time.time() - t0, 1),
           "wave_route_in_this_build": has_route, "workloads": {}}

    def long_batch(lens, R):
        off = np.zeros(len(lens) + 1, dtype=np.int64)
        off[1:] = np.cumsum(lens.astype(np.int64))
        d_off = torch.from_numpy(off).to(dev)
        d_reads = torch.empty(int(off[-1]) + 64, dtype=torch.uint8, device=dev)
        S.synth_long_reads_device(P, R, 0, len(lens), d_off, int(off[-1]), d_reads)
        return d_reads, d_off, len(lens), False, int(off[-1])

    def workload(name):
        if name == "a":
            R = S.read_params(0x5C2B0020, host_pct=50, sub_per_10k=200, n_read_pct=1)
            lens = B.long_read_lengths(R.seed, 0, n_long)
            return (f"{n_long} long reads, the length law of bench.py --workload ont (mean {lens.mean():.0f}, max {int(lens.max())} bases)",) + long_batch(lens, R)
        if name == "b":
            R = S.read_params(0x5C2B0021, host_pct=50, sub_per_10k=200, n_read_pct=1)
            return (f"{n_long} reads of 10 000 bases",) + long_batch(np.full(n_long, 10_000, dtype=np.uint32), R)
        R = S.read_params(0x5C2B0030)
        d_reads = torch.empty(n_short * R.read_len + 64, dtype=torch.uint8, device=dev)
        d_off = torch.empty(n_short + 1, dtype=torch.int64, device=dev)
        S.synth_reads_device(P, R, 0, n_short, d_reads, d_off)
        return (f"configs[4] stand-in: {n_short // 2} pairs of 2x{R.read_len} bp", d_reads, d_off, n_short, True, n_short * R.read_len)

    for w in a.workloads.split(","):
        desc, d_reads, d_off, n_rec, paired, n_bases = workload(w)
        n_units = n_rec // 2 if paired else n_rec
        d_out = torch.zeros((n_units, 4), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        rec = {"workload": desc, "n_bases": n_bases, "forms": {}}
        first = None
        for form in ("plain", "hits"):
            rec["forms"][form] = {}
            for thr in (THRESHOLDS if has_route else [-1]):
                o = db.opts()
                if has_route:
                    o.long_unit_bases = thr
                ms, ms_long, wall, st, extra = [], [], [], None, {}
                for i in range(a.launches + 1):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    if form == "plain":
                        st = db.classify_device(d_reads, d_off, n_rec, paired, d_out, o)
                    else:
                        st, (po, pe, nu, ne, h) = db.classify_device_hits(d_reads, d_off, n_rec, paired, d_out, o, to_host=False)
                        extra = {"n_entries": ne, "n_redone": K.K2Db.hits_redone(h)}
                        K.K2Db.free_hits(h)
                    torch.cuda.synchronize()
                    if i:
                        ms.append(st["ms_classify"]); ms_long.append(st.get("ms_long", 0.0)); wall.append((time.perf_counter() - t) * 1e3)
                res = d_out.cpu().numpy().copy()
                first = res if first is None else first
                rec["forms"][form][str(thr)] = dict(
                    {"ms_classify_median": round(statistics.median(ms), 3), "ms_classify_min": round(min(ms), 3), "ms_classify_max": round(max(ms), 3),
                     "ms_long_median": round(statistics.median(ms_long), 3), "ms_call_median": round(statistics.median(wall), 3),
                     "n_long_units": st.get("n_long_units", 0), "n_classified": st["n_classified"], "n_probes": st["n_probes"], "n_kmers": st["n_kmers"],
                     "n_overflow": st["n_overflow"], "results_equal_first_mode": bool((res == first).all())}, **extra)
                print(w, form, thr, rec["forms"][form][str(thr)], file=sys.stderr, flush=True)
        out["workloads"][w] = rec
        del d_reads, d_off, d_out
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
