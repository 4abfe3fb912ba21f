"""Cost of Kraken 2's hit lists (k_k2_classify's HITS instance, sh_k2_classify_ex_device) on the configs[4] stand-in of
bench.py (--workload k2: synthetic 2x150 bp pairs against a 2e9-cell table holding the CHM13-sized synthetic reference under
Homo sapiens plus filler keys), the same setup as scripts/k2_options_speed.py.

Modes, on the same pairs and table: the default path (default kernel instance) and the hit lists.  Each: one warm-up launch,
then the median of --launches launches of sh_k2_stats.ms_classify (HIP events around the first-pass kernel) and of the whole
call's wall time (hit lists: allocation, scan of the counts, overflow pass, compaction; the lists stay in HBM).  Prints one JSON
object; --out writes it too.  The end-to-end Kraken run is bench.py --workload e2e-k2.

    python scripts/k2_hits_speed.py [--launches 7] [--small] [--out profiles/k2_hits.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B  # noqa: E402
from scrubby_amd import k2 as K  # noqa: E402
from scrubby_amd import lib as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="5 x 1 Mb reference, 200 000 records, 12 M cells (a rehearsal)")
    ap.add_argument("--out")
    a = ap.parse_args()
    S.require_gpu()
    dev = torch.device("cuda:0")
    contigs = [1_000_000] * 5 if a.small else B.CHM13_CONTIGS
    n_rec = 200_000 if a.small else 40_000_000
    cells = 12_000_017 if a.small else 2_000_000_000
    P = S.ref_params(B.REF_SEED, contigs)
    R = S.read_params(0x5C2B0030)
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
    d_reads = torch.empty(n_rec * R.read_len + 64, dtype=torch.uint8, device=dev)
    d_off = torch.empty(n_rec + 1, dtype=torch.int64, device=dev)
    S.synth_reads_device(P, R, 0, n_rec, d_reads, d_off)
    d_out = torch.zeros((n_rec // 2, 4), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    setup_s = time.time() - t0

    out = {"workload": f"configs[4] stand-in (bench.py --workload k2): {n_rec // 2} pairs of 2x{R.read_len} bp, {cells} cells, "
                       f"k=35 l=31, confidence 0, minimum-hit-groups 2", "launches": a.launches, "setup_s": round(setup_s, 1), "modes": {}}
    o = db.opts()
    results = {}
    for name in ("default", "hits", "default_again"):
        ms, wall, st, extra = [], [], None, {}
        for i in range(a.launches + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            if name.startswith("default"):
                st = db.classify_device(d_reads, d_off, n_rec, True, d_out, o)
            else:
                st, (po, pe, nu, ne, h) = db.classify_device_hits(d_reads, d_off, n_rec, True, d_out, o, to_host=False)
                extra = {"n_entries": ne, "entries_per_pair": round(ne / nu, 3), "n_redone": K.K2Db.hits_redone(h)}
                K.K2Db.free_hits(h)
            torch.cuda.synchronize()
            if i:
                ms.append(st["ms_classify"]); wall.append((time.perf_counter() - t) * 1e3)
        results[name] = d_out.cpu().numpy().copy()
        out["modes"][name] = dict({"ms_classify_median": round(statistics.median(ms), 3), "ms_classify": [round(x, 3) for x in ms],
                                   "ms_call_median": round(statistics.median(wall), 3), "n_classified": st["n_classified"],
                                   "n_probes": st["n_probes"], "n_kmers": st["n_kmers"], "n_overflow": st["n_overflow"]}, **extra)
    base = out["modes"]["default"]
    for m in out["modes"].values():
        m["vs_default"] = round(m["ms_classify_median"] / base["ms_classify_median"], 3)
        m["call_vs_default"] = round(m["ms_call_median"] / base["ms_call_median"], 3)
    out["results_identical"] = bool((results["default"] == results["hits"]).all())
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
