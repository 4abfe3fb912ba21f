"""The Kraken arm's k-mer distribution (bracken-build on the GPU): the codes kernel and the window kernel of
sh_k2_distrib_add_device, on the synthetic table of scripts/k2_long_speed.py (the stand-in database of bench.py --workload k2:
2e9 cells, the CHM13-sized synthetic reference under Homo sapiens plus filler keys).

Libraries, resident in HBM, read length 150:
  a   40 records of 5 Mb cut from the synthetic reference (about 200 Mb), alternately under Homo sapiens and under a bacterial
      species: every window holds one taxon, the easy case (a genome against its own database);
  b   a second synthetic sequence of 400 Mb, inserted in tiles of 500 bases under 997 bacterial species in rotation, as 80 records
      of 5 Mb under the first of them: a window that straddles a tile border holds two taxa (and k-mers of no taxon), so the calls
      change every few hundred windows and ResolveTree runs.
For each stretch S (SCRUBBY_HIP_K2_DISTRIB_STRETCH): one warm-up call, then --launches calls into a reset accumulator; the medians
of the two kernels' times (sh_k2_distrib_last_ms), windows per second and n_big are recorded, and the distributions of all S must
be equal.

What a user has to do today, on an 8 Mb slice (4 Mb of library a, 4 Mb of library b): materialise every window as a 150-base read (on the device),
run the windows through sh_k2_classify_ex_device with min_hit_groups = 1, tally (genome, call) on the host.  Its distribution must
equal the accumulator's on that slice; the ratio of the two times is recorded beside the absolute figures.
Prints one JSON object; --out writes it too.

    python scripts/k2_bracken_speed.py [--launches 7] [--small] [--out profiles/k2_bracken.json]
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

STRETCHES = [32, 64, 128, 256, 1024]
READ_LEN = 150


def as_map(ent):
    return {(int(g), int(m)): int(w) for g, m, w in ent}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="5 x 1 Mb reference, 12 M cells, a 4 Mb library, a 0.4 Mb slice (a rehearsal)")
    ap.add_argument("--out")
    a = ap.parse_args()
    S.require_gpu()
    dev = torch.device("cuda:0")
    contigs = [1_000_000] * 5 if a.small else B.CHM13_CONTIGS
    cells = 12_000_017 if a.small else 2_000_000_000
    n_rec, rec_len = (8, 500_000) if a.small else (40, 5_000_000)
    slice_rec, slice_len = (2, 200_000) if a.small else (2, 4_000_000)
    P = S.ref_params(B.REF_SEED, contigs)
    G = P.genome_len
    t0 = time.time()
    parents, externals, names, ranks, ids = B.k2_taxonomy(2_000 if a.small else 50_000, 0x5C2B0030)
    db = K.K2Db.create(K.default_opts(), cells, parents, externals, names, ranks)
    d_ref = torch.empty(G + 64, dtype=torch.uint8, device=dev)
    S.synth_ref_device(P, 0, G, d_ref)
    db.insert_sequence_device(d_ref, G, ids["Homo sapiens"])
    # the library: records cut from the reference at even spacing
    step = (G - rec_len) // n_rec
    d_lib = torch.cat([d_ref[i * step: i * step + rec_len] for i in range(n_rec)] + [torch.full((64,), ord("N"), dtype=torch.uint8, device=dev)])
    del d_ref
    torch.cuda.empty_cache()
    # library b: a sequence of its own in tiles of 500 bases under rotating species
    species = [i for i, r in enumerate(ranks) if r == "species" and i > ids["Bacteria"]][:997]
    G2, tile = (4_000_000, 500) if a.small else (400_000_000, 500)
    P2 = S.ref_params(0x5C2B0041, [G2])
    d_seq2 = torch.empty(G2 + 64, dtype=torch.uint8, device=dev)
    S.synth_ref_device(P2, 0, G2, d_seq2)
    d_seq2[G2:] = ord("N")
    n_tiles = G2 // tile
    d_toff = torch.arange(n_tiles + 1, dtype=torch.int64, device=dev) * tile
    d_ttaxa = torch.tensor(species, dtype=torch.int32, device=dev)[torch.arange(n_tiles, device=dev) % len(species)].contiguous()
    db.insert_library_device(d_seq2, d_toff, d_ttaxa, n_tiles)
    db.insert_random(0x5C2B0031, max(int(0.70 * cells) - db.info()["size"], 0), ids["Bacteria"], len(parents) - 1)
    bact = next(i for i, r in enumerate(ranks) if r == "species" and i > ids["Bacteria"])
    taxa = [ids["Homo sapiens"] if i % 2 == 0 else bact for i in range(n_rec)]
    d_off = torch.arange(n_rec + 1, dtype=torch.int64, device=dev) * rec_len
    d_taxa = torch.tensor(taxa + [0], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    n_bases = n_rec * rec_len
    out = {"table": f"{cells} cells, k=35 l=31", "library": f"{n_rec} records of {rec_len} bases ({n_bases} bases), read length {READ_LEN}",
           "launches": a.launches, "setup_s": round(time.time() - t0, 1), "stretch_default": None, "stretches": {}}
    os.environ.pop("SCRUBBY_HIP_K2_DISTRIB_STRETCH", None)
    out["stretch_default"] = K.distrib_stretch()
    d = K.KmerDistrib(db, READ_LEN)

    def sweep(d_bases, d_offsets, d_taxa_, n):
        res, first = {}, None
        for s in STRETCHES:
            os.environ["SCRUBBY_HIP_K2_DISTRIB_STRETCH"] = str(s)
            assert K.distrib_stretch() == s
            mc, mw, st = [], [], None
            for i in range(a.launches + 1):
                d.reset()
                st = d.add_device(d_bases, d_offsets, d_taxa_, n)
                if i:
                    c, w = d.last_ms()
                    mc.append(c); mw.append(w)
            ent = as_map(d.entries())
            first = ent if first is None else first
            c, w = statistics.median(mc), statistics.median(mw)
            res[str(s)] = {"ms_codes_median": round(c, 3), "ms_windows_median": round(w, 3), "ms_windows_min": round(min(mw), 3), "ms_windows_max": round(max(mw), 3),
                           "windows_per_s_window_kernel": round(st["n_windows"] / (w * 1e-3)), "windows_per_s_both": round(st["n_windows"] / ((c + w) * 1e-3)),
                           "n_windows": st["n_windows"], "n_items": st["n_items"], "n_big": st["n_big"], "n_entries": len(ent),
                           "distribution_equal_first_stretch": ent == first}
            print(s, res[str(s)], file=sys.stderr, flush=True)
        return res

    out["stretches"] = sweep(d_lib, d_off, d_taxa, n_rec)
    nb_rec = G2 // rec_len
    d_boff = torch.arange(nb_rec + 1, dtype=torch.int64, device=dev) * rec_len
    d_btaxa = torch.tensor([species[0]] * nb_rec + [0], dtype=torch.int32, device=dev)
    out["library_b"] = f"{nb_rec} records of {rec_len} bases of a sequence inserted in tiles of {tile} bases under {len(species)} species"
    out["stretches_b"] = sweep(d_seq2, d_boff, d_btaxa, nb_rec)
    os.environ.pop("SCRUBBY_HIP_K2_DISTRIB_STRETCH", None)

    # ---- what a user does today, on a slice: every window as a read through the classifier, tallied on the host
    assert slice_rec == 2
    slice_taxa = [taxa[0], species[0]]          # one record of library a, one of library b
    d_soff = torch.arange(slice_rec + 1, dtype=torch.int64, device=dev) * slice_len
    d_slice = torch.cat([d_lib[:slice_len], d_seq2[:slice_len], torch.full((64,), ord("N"), dtype=torch.uint8, device=dev)])
    d_staxa = torch.tensor(slice_taxa + [0], dtype=torch.int32, device=dev)
    ms_acc = []
    for i in range(a.launches + 1):
        d.reset()
        st = d.add_device(d_slice, d_soff, d_staxa, slice_rec)
        if i:
            ms_acc.append(st["ms"])
    acc = as_map(d.entries())
    o = db.opts()
    o.min_hit_groups = 1
    o.long_unit_bases = -1
    n_win_rec = slice_len - READ_LEN + 1
    n_win = slice_rec * n_win_rec
    ms_mat, ms_cls, ms_tally = [], [], []
    today = None
    for i in range(a.launches + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        reads = torch.cat([d_slice[r * slice_len: (r + 1) * slice_len].unfold(0, READ_LEN, 1).reshape(-1) for r in range(slice_rec)]
                          + [torch.full((64,), ord("N"), dtype=torch.uint8, device=dev)])
        roff = torch.arange(n_win + 1, dtype=torch.int64, device=dev) * READ_LEN
        d_res = torch.zeros((n_win, 4), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        cst = db.classify_device(reads, roff, n_win, False, d_res, o)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        calls = d_res[:, 1].cpu().numpy().astype(np.int64)
        genome = np.repeat(np.array(slice_taxa, dtype=np.int64), n_win_rec)
        keys, cnt = np.unique(genome << 32 | calls, return_counts=True)
        today = {(int(k >> 32), int(k & 0xffffffff)): int(c) for k, c in zip(keys, cnt)}
        t3 = time.perf_counter()
        del reads, roff, d_res
        if i:
            ms_mat.append((t1 - t) * 1e3); ms_cls.append(cst["ms_classify"]); ms_tally.append((t3 - t2) * 1e3)
    whole = statistics.median(ms_mat) + statistics.median(ms_cls) + statistics.median(ms_tally)
    out["today_on_a_slice"] = {"slice": f"{slice_len} bases of library a and of library b, {n_win} windows", "ms_accumulator_median": round(statistics.median(ms_acc), 3),
                               "ms_materialise_median": round(statistics.median(ms_mat), 3), "ms_classify_median": round(statistics.median(ms_cls), 3),
                               "ms_host_tally_median": round(statistics.median(ms_tally), 3), "ms_today_total": round(whole, 3),
                               "ratio_classify_kernel_over_accumulator": round(statistics.median(ms_cls) / statistics.median(ms_acc), 2),
                               "ratio_today_total_over_accumulator": round(whole / statistics.median(ms_acc), 2), "distribution_equal": today == acc,
                               "n_entries": len(acc)}
    print(out["today_on_a_slice"], file=sys.stderr, flush=True)
    d.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    assert all(v["distribution_equal_first_stretch"] for w in ("stretches", "stretches_b") for v in out[w].values()) and out["today_on_a_slice"]["distribution_equal"]


if __name__ == "__main__":
    main()
