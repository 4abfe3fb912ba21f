"""Speed of database inspection (DESIGN.md §7 "Database inspection").

counts    sh_k2_value_counts_device with statistics (so the call ends in a synchronise) on tables of --cells cells (2^31 = 8 GB, the
          size of the configs[4] stand-in) filled to load 0.7 by sh_k2_insert_random: (a) values uniform over 17 taxa, (b) one taxon,
          (c) 70 001 taxa with half of the cells on 20 hot ids that lie BEHIND the LDS bins (ids 5000..5019: every one of them is a
          64-bit add in HBM), (c_low) the same with the hot ids inside the bins (ids 2..21, where breadth-first ids put hot LCAs).
          Wall time of the whole call; median, minimum and maximum of --launches runs after one warm-up, and the device time the call
          itself reports.  --verify compares every table's counts with NumPy on an export of its cells.
read      the yardstick, not the code under test: torch.sum over an int32 tensor of as many elements in the same process on the same
          device, timed the same way.  The ratios of (a), (b), (c) to it and (b) / (a) are recorded.
cli       `scrubby-hip k2-inspect` on table (a) saved to --work, split as its result struct splits it (opening 8 GB from disk is most of it).

    python scripts/k2_inspect_speed.py [--launches 7] [--small] [--verify] [--no-cli] [--work DIR] [--out profiles/k2_inspect.json]
"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scrubby_amd import k2 as K  # noqa: E402
from scrubby_amd import lib as S  # noqa: E402


def summary(xs):
    return {"median_s": round(statistics.median(xs), 6), "min_s": round(min(xs), 6), "max_s": round(max(xs), 6), "runs": len(xs)}


def timed(fn, runs):
    ts = []
    for _ in range(runs + 1):          # one warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return summary(ts[1:])


def flat_taxonomy(n):
    """n nodes: the empty node, the root, and n - 2 species under it"""
    return [0, 0] + [1] * (n - 2), list(range(n)), [""] + ["t%d" % i for i in range(1, n)], ["", "no rank"] + ["species"] * (n - 2)


def heap_taxonomy(n):
    return [0, 0] + [i // 2 for i in range(2, n)], list(range(n)), [""] + ["t%d" % i for i in range(1, n)], ["", "no rank"] + ["no rank"] * (n - 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--cells", type=int, default=1 << 31)
    ap.add_argument("--small", action="store_true", help="a rehearsal: 2^24 cells")
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--work", default="/tmp/k2_inspect_speed")
    ap.add_argument("--out")
    a = ap.parse_args()
    S.require_gpu()
    cap = (1 << 24) if a.small else a.cells
    n_fill = int(cap * 0.7)
    res = {"workload": {"cells": cap, "bytes": cap * 4, "load_asked": 0.7}, "launches": a.launches}

    x = torch.full((cap,), 3, dtype=torch.int32, device="cuda")

    def read():
        x.sum()
        torch.cuda.synchronize()

    res["read_torch_sum_int32"] = timed(read, a.launches)
    res["read_torch_sum_int32"]["gb_per_s"] = round(cap * 4 / res["read_torch_sum_int32"]["median_s"] / 1e9, 1)
    del x
    torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)

    cases = [("a_uniform_17_taxa", 5, flat_taxonomy(18), [(n_fill, 1, 17)]),
             ("b_one_taxon", 2, flat_taxonomy(3), [(n_fill, 2, 2)]),
             ("c_70001_taxa_hot_behind_the_bins", 17, heap_taxonomy(70_001), [(n_fill // 2, 1, 70_000), (n_fill - n_fill // 2, 5000, 5019)]),
             ("c_low_70001_taxa_hot_inside_the_bins", 17, heap_taxonomy(70_001), [(n_fill // 2, 1, 70_000), (n_fill - n_fill // 2, 2, 21)])]
    for name, vb, tax, fills in cases:
        o = K.default_opts()
        o.value_bits = vb
        d = K.K2Db.create(o, cap, *tax)
        for i, (n, lo, hi) in enumerate(fills):
            d.insert_random(0x5C2B1000 + i, n, lo, hi)
        n_nodes = len(tax[0])
        out = torch.empty(n_nodes, dtype=torch.int64, device="cuda")
        st = {}

        def count():
            st.update(d.value_counts_device(out, stats=True))

        r = timed(count, a.launches)
        counts = out.cpu().numpy().view(np.uint64)
        r.update(device_ms=round(st["ms"], 4), n_occupied=st["n_occupied"], n_bad_values=st["n_bad_values"], load=round(st["n_occupied"] / cap, 4),
                 n_nodes=n_nodes, taxa_with_minimizers=int((counts != 0).sum()), largest_count=int(counts.max()),
                 gb_per_s=round(cap * 4 / r["median_s"] / 1e9, 1), ratio_to_read=round(r["median_s"] / res["read_torch_sum_int32"]["median_s"], 3))
        assert int(counts.sum()) == st["n_occupied"] and st["n_bad_values"] == 0
        if a.verify:
            cells = d.export()[0]
            occ = cells != 0
            exp = np.bincount(cells[occ] & np.uint32((1 << vb) - 1), minlength=n_nodes).astype(np.uint64)
            assert np.array_equal(counts, exp), name
            r["verified_against_numpy"] = True
            del cells, occ, exp
        res[name] = r
        print(json.dumps({name: r}), flush=True)
        if name.startswith("a_") and not a.no_cli:
            shutil.rmtree(a.work, ignore_errors=True)
            os.makedirs(a.work)
            t0 = time.time()
            d.save(a.work)
            s_save = time.time() - t0
            d.close()
            t0 = time.time()
            p = subprocess.run([os.path.join(ROOT, "scrubby_amd", "scrubby-hip"), "k2-inspect", "-d", a.work, "-o", os.path.join(a.work, "report.txt")],
                               capture_output=True, text=True)
            wall = time.time() - t0
            m = re.search(r"open ([0-9.]+) s, count ([0-9.]+) s, report ([0-9.]+) s, total ([0-9.]+) s", p.stderr)
            res["cli_k2_inspect_on_a"] = {"returncode": p.returncode, "wall_s": round(wall, 3), "s_save_before_it": round(s_save, 3),
                                          "report_lines": sum(1 for _ in open(os.path.join(a.work, "report.txt"))) if p.returncode == 0 else 0}
            if m:
                res["cli_k2_inspect_on_a"].update(s_open=float(m.group(1)), s_count=float(m.group(2)), s_report=float(m.group(3)), s_total=float(m.group(4)))
            else:
                res["cli_k2_inspect_on_a"]["stderr"] = p.stderr[-500:]
            shutil.rmtree(a.work, ignore_errors=True)
            print(json.dumps({"cli_k2_inspect_on_a": res["cli_k2_inspect_on_a"]}), flush=True)
        else:
            d.close()
        del out
        torch.cuda.empty_cache()
    res["ratio_b_over_a"] = round(res["b_one_taxon"]["median_s"] / res["a_uniform_17_taxa"]["median_s"], 3)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
