"""Classify time of kraken2's --minimum-base-quality and --quick on the configs[4] stand-in of bench.py (--workload k2: 20 M
synthetic 2x150 bp pairs against a 2e9-cell table holding the CHM13-sized synthetic reference under Homo sapiens plus filler keys).

Modes, all on the same pairs and table: the default path (options off: the default kernel instance); --minimum-base-quality 20
(QMASK instance) over three seeded sets of Phred qualities: none below 20 (the cost of the switch alone), a low-quality run of 3-30
bases in every second read, and 10 % of the bases low at random (nearly every k-mer then covers a masked base); --quick (QUICK
instance); and --quick with the low-quality runs.  Each mode: one warm-up launch, then the median of
--launches launches of sh_k2_stats.ms_classify (HIP events around the classify kernels).  Prints one JSON object; --out writes it too.

    python scripts/k2_options_speed.py [--launches 7] [--small] [--out profiles/k2_options.json]
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


def device_quals(n_rec, read_len, kind, seed, dev):
    """Phred+33 on the device, read_len per record and 64 padding bytes: Q20-Q41, plus (kind "runs") one run of 3-30 bases at
    Q2-Q14 in every second read, or (kind "uniform10") 10 % of the bases at Q2-Q19"""
    g = torch.Generator(device=dev); g.manual_seed(seed)
    n = n_rec * read_len
    q = torch.full((n + 64,), 0xFF, dtype=torch.uint8, device=dev)
    good = torch.randint(20 + 33, 42 + 33, (n,), dtype=torch.uint8, device=dev, generator=g)
    if kind == "runs":
        pos = torch.arange(read_len, device=dev, dtype=torch.int16)[None, :]
        has = torch.rand(n_rec, device=dev, generator=g)[:, None] < 0.5
        beg = torch.randint(0, read_len, (n_rec, 1), dtype=torch.int16, device=dev, generator=g)
        end = beg + torch.randint(3, 31, (n_rec, 1), dtype=torch.int16, device=dev, generator=g)
        low = (has & (pos >= beg) & (pos < end)).reshape(-1)
        del pos, has, beg, end
        bad = torch.randint(2 + 33, 15 + 33, (n,), dtype=torch.uint8, device=dev, generator=g)
        good = torch.where(low, bad, good)
    elif kind == "uniform10":
        low = torch.rand(n, device=dev, generator=g) < 0.10
        bad = torch.randint(2 + 33, 20 + 33, (n,), dtype=torch.uint8, device=dev, generator=g)
        good = torch.where(low, bad, good)
    q[:n] = good
    return q


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
    n_bases = n_rec * R.read_len
    d_reads = torch.empty(n_bases + 64, dtype=torch.uint8, device=dev)
    d_off = torch.empty(n_rec + 1, dtype=torch.int64, device=dev)
    S.synth_reads_device(P, R, 0, n_rec, d_reads, d_off)
    d_out = torch.zeros((n_rec // 2, 4), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    setup_s = time.time() - t0

    # mode: (options, qualities)
    modes = {"default": ({}, None),
             "min_base_quality_20_none_below": ({"min_base_quality": 20}, "none"),
             "min_base_quality_20_runs": ({"min_base_quality": 20}, "runs"),
             "min_base_quality_20_uniform10": ({"min_base_quality": 20}, "uniform10"),
             "quick": ({"quick": 1}, None),
             "quick_and_min_base_quality_20_runs": ({"quick": 1, "min_base_quality": 20}, "runs")}
    out = {"workload": f"configs[4] stand-in (bench.py --workload k2): {n_rec // 2} pairs of 2x{R.read_len} bp, {cells} cells, "
                       f"k=35 l=31, confidence 0, minimum-hit-groups 2", "launches": a.launches, "setup_s": round(setup_s, 1),
           "qualities": {"none": "Q20-Q41", "runs": "Q20-Q41, one run of 3-30 bases at Q2-Q14 in every second read",
                         "uniform10": "Q20-Q41, 10 % of the bases Q2-Q19 at random"}, "modes": {}}
    quals = {}
    for name, (kw, qk) in modes.items():
        o = db.opts()
        for k, v in kw.items():
            setattr(o, k, v)
        if qk is not None and qk not in quals:
            quals.clear()
            torch.cuda.empty_cache()
            quals[qk] = device_quals(n_rec, R.read_len, qk, 0x5C2B0032, dev)
        dq = quals[qk] if qk is not None else None
        ms, st = [], None
        for i in range(a.launches + 1):
            st = db.classify_device(d_reads, d_off, n_rec, True, d_out, o, d_quals=dq)
            if i:
                ms.append(st["ms_classify"])
        res = d_out.cpu().numpy().view(K.RESULT_DTYPE).reshape(-1)
        out["modes"][name] = {"ms_classify_median": round(statistics.median(ms), 3), "ms_classify": [round(x, 3) for x in ms],
                              "n_classified": st["n_classified"], "n_probes": st["n_probes"], "n_kmers": st["n_kmers"],
                              "n_masked_bases": st["n_masked_bases"], "n_overflow": st["n_overflow"],
                              "human_pairs": int((res["taxid"] == 9606).sum())}
    base = out["modes"]["default"]["ms_classify_median"]
    for name, m in out["modes"].items():
        m["vs_default"] = round(m["ms_classify_median"] / base, 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
