"""Translated search on the configs[4] stand-in: a protein database (k 15, l 12) filled with sh_k2_insert_random to load 0.7 and
synthetic 2x150 bp pairs resident in HBM (the reads of scripts/k2_options_speed.py).  Nothing exists to compare the protein path
against, so there is no pass mark: the figures are written down with what bounds them.

One warm-up launch, then --launches launches of sh_k2_classify_ex_device; per launch sh_k2_stats gives ms_translate (k_k2_translate)
and ms_classify (the protein form of k_k2_classify, its BIG pass included).  Recorded: the medians, smallest and largest of both,
probes and k-mers per unit, reads per second over ms_translate + ms_classify, and the roofline share: probes per second of
ms_classify over the gather ceiling the DNA path is measured against (DESIGN.md §7 "Bound": 49 G probes/s).
Prints one JSON object; --out writes it too.

    python scripts/k2_tx_speed.py [--launches 5] [--pairs 10000000] [--cells 2000000000] [--small] [--out FILE]
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

GATHER_CEILING = 49e9       # probes/s, DESIGN.md §7 "Bound"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--cells", type=int, default=2_000_000_000)
    ap.add_argument("--small", action="store_true", help="12 M cells, 100 000 pairs (a rehearsal)")
    ap.add_argument("--out")
    a = ap.parse_args()
    S.require_gpu()
    dev = torch.device("cuda:0")
    cells = 12_000_017 if a.small else a.cells
    n_pairs = 100_000 if a.small else a.pairs
    contigs = [1_000_000] * 5 if a.small else B.CHM13_CONTIGS
    t0 = time.time()
    parents, externals, names, ranks, ids = B.k2_taxonomy(2_000 if a.small else 50_000, 0x5C2B0030)
    db = K.K2Db.create(K.default_protein_opts(), cells, parents, externals, names, ranks)
    db.insert_random(0x5C2B0041, int(0.70 * cells), ids["Bacteria"], len(parents) - 1)
    P = S.ref_params(B.REF_SEED, contigs)
    R = S.read_params(0x5C2B0030)
    n_rec = 2 * n_pairs
    d_reads = torch.empty(n_rec * R.read_len + 64, dtype=torch.uint8, device=dev)
    d_off = torch.empty(n_rec + 1, dtype=torch.int64, device=dev)
    S.synth_reads_device(P, R, 0, n_rec, d_reads, d_off)
    d_out = torch.zeros((n_pairs, 4), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    setup_s = round(time.time() - t0, 1)
    ms_tx, ms_cl, wall, st = [], [], [], None
    for i in range(a.launches + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        st = db.classify_device(d_reads, d_off, n_rec, True, d_out)
        torch.cuda.synchronize()
        if i:
            ms_tx.append(st["ms_translate"]); ms_cl.append(st["ms_classify"]); wall.append((time.perf_counter() - t) * 1e3)
    mt, mc = statistics.median(ms_tx), statistics.median(ms_cl)
    info = db.info()
    out = {
        "table": f"{cells} cells, protein, k=15 l=12, load {info['size'] / cells:.3f} (sh_k2_insert_random), confidence 0, minimum-hit-groups 2",
        "workload": f"{n_pairs} synthetic pairs of 2x{R.read_len} bp, resident in HBM", "launches": a.launches, "setup_s": setup_s,
        "ms_translate": {"median": round(mt, 3), "min": round(min(ms_tx), 3), "max": round(max(ms_tx), 3)},
        "ms_classify": {"median": round(mc, 3), "min": round(min(ms_cl), 3), "max": round(max(ms_cl), 3)},
        "ms_call_median": round(statistics.median(wall), 3),
        "probes_per_unit": round(st["n_probes"] / n_pairs, 2), "kmers_per_unit": round(st["n_kmers"] / n_pairs, 2),
        "n_classified": st["n_classified"], "n_overflow": st["n_overflow"],
        "reads_per_s": round(n_rec / ((mt + mc) * 1e-3)),
        "translate_bytes": {"read": n_rec * R.read_len, "written": 2 * n_rec * (R.read_len - 2)},
        "translate_GBps": round((n_rec * R.read_len + 2 * n_rec * (R.read_len - 2)) / (mt * 1e-3) / 1e9, 1),
        "probes_per_s": round(st["n_probes"] / (mc * 1e-3)),
        "roofline_share_of_gather_ceiling": round(st["n_probes"] / (mc * 1e-3) / GATHER_CEILING, 3),
        "gather_ceiling_probes_per_s": GATHER_CEILING,
    }
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
