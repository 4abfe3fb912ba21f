"""Speed of the Kraken arm's database build (DESIGN.md §7 "Database build").

kernels   sh_k2_insert_library_device (one launch per batch) against the only way the parent commit had to do the same,
          sh_k2_insert_sequence_device once per record, on (a) one synthetic sequence of 200 Mb and (b) the same bases as 100 000
          records of 2 kb, each into a fresh table of the same size; wall time of the whole call(s), synchronisation included
          (that is what the per-record path pays once per record); median, minimum and maximum of --launches runs.  The per-record
          path of (b) costs about a millisecond per call, so it is timed on the first --old-records records (10 000) and
          its figure for all of them is that time scaled by their number (`scaled_median_s`); the table says which is which.  The new kernel
          is also run with other segment lengths (SCRUBBY_HIP_K2_SEG) to record the choice of 1024.
e2e       `scrubby-hip k2-build --taxid 9606` on a FASTA of the synthetic CHM13v2-sized reference bench.py uses (3.1 Gb, written
          from sh_synth_ref_device): the seconds per phase the command prints, and the fill's insert rate.

    python scripts/k2_build_speed.py [--launches 7] [--small] [--no-e2e] [--work DIR] [--out profiles/k2_build.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B  # noqa: E402
from scrubby_amd import k2 as K  # noqa: E402
from scrubby_amd import lib as S  # noqa: E402


def summary(xs):
    return {"median_s": round(statistics.median(xs), 5), "min_s": round(min(xs), 5), "max_s": round(max(xs), 5), "runs": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="a rehearsal: 8 Mb, 4 000 records, a 5 x 1 Mb reference")
    ap.add_argument("--old-records", type=int, default=10_000, help="records of (b) the per-record path is timed on")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--work", default="/tmp/k2_build_speed")
    ap.add_argument("--out")
    a = ap.parse_args()
    S.require_gpu()
    dev = torch.device("cuda:0")
    n_rec, rec_len = (4_000, 2_000) if a.small else (100_000, 2_000)
    n = n_rec * rec_len
    cells = 12_000_017 if a.small else 300_000_007
    P = S.ref_params(B.REF_SEED, [n])
    d_ref = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    S.synth_ref_device(P, 0, n, d_ref)
    d_ref[n:] = ord("N")
    d_off1 = torch.tensor([0, n], dtype=torch.int64, device=dev)
    d_tax1 = torch.tensor([2], dtype=torch.int32, device=dev)
    d_offn = torch.arange(0, n + 1, rec_len, dtype=torch.int64, device=dev)
    d_taxn = torch.full((n_rec,), 2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    n_old = min(a.old_records, n_rec)

    def fresh():
        return K.K2Db.create(K.default_opts(), cells, [0, 0, 1], [0, 1, 9606], ["", "root", "Homo sapiens"], ["", "no rank", "species"])

    def timed(fn, runs):
        ts, info = [], None
        for i in range(runs + 1):          # one warm-up
            db = fresh()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = fn(db)
            ts.append(time.perf_counter() - t0)
            info = dict(info or {}, size=db.info()["size"])
            db.close()
        return dict(summary(ts[1:]), **info)

    def old_one(db):
        return {"n_runs": db.insert_sequence_device(d_ref, n, 2)}

    def old_many(db):
        base, r = d_ref.data_ptr(), 0
        import ctypes as C
        L, out = S.load(), C.c_uint64()
        for i in range(n_old):
            S.check(L.sh_k2_insert_sequence_device(db.h, C.c_void_p(base + i * rec_len), C.c_uint64(rec_len), C.c_uint32(2), None, C.byref(out)))
            r += out.value
        return {"n_runs": r}

    def new_one(db):
        return db.insert_library_device(d_ref, d_off1, d_tax1, 1)

    def new_many(db):
        return db.insert_library_device(d_ref, d_offn, d_taxn, n_rec)

    res = {"workload": {"bases": n, "records_b": n_rec, "record_len_b": rec_len, "cells": cells}, "launches": a.launches}
    res["a_one_sequence"] = {"per_record_kernel": timed(old_one, a.launches), "library_kernel": timed(new_one, a.launches)}
    res["b_many_records"] = {"per_record_kernel": timed(old_many, a.launches), "library_kernel": timed(new_many, a.launches)}
    ob = res["b_many_records"]["per_record_kernel"]
    ob["records_timed"] = n_old
    ob["scaled_median_s"] = round(ob["median_s"] * n_rec / n_old, 4)
    ob["per_call_us"] = round(1e6 * ob["median_s"] / n_old, 1)
    res["a_one_sequence"]["ratio_old_over_new"] = round(res["a_one_sequence"]["per_record_kernel"]["median_s"] / res["a_one_sequence"]["library_kernel"]["median_s"], 3)
    res["b_many_records"]["ratio_old_over_new"] = round(ob["scaled_median_s"] / res["b_many_records"]["library_kernel"]["median_s"], 1)
    res["segment_sweep"] = {}
    for seg in (128, 256, 512, 1024, 2048, 4096):
        os.environ["SCRUBBY_HIP_K2_SEG"] = str(seg)
        res["segment_sweep"][str(seg)] = {"a_one_sequence": timed(new_one, a.launches), "b_many_records": timed(new_many, a.launches)}
    del os.environ["SCRUBBY_HIP_K2_SEG"]
    del d_ref
    torch.cuda.empty_cache()
    print(json.dumps({k: res[k] for k in ("a_one_sequence", "b_many_records")}), flush=True)

    if not a.no_e2e:
        contigs = [1_000_000] * 5 if a.small else B.CHM13_CONTIGS
        P = S.ref_params(B.REF_SEED, contigs)
        G = P.genome_len
        os.makedirs(a.work, exist_ok=True)
        fa = os.path.join(a.work, "ref.fa")
        t0 = time.time()
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
        t_write = time.time() - t0
        exe = os.path.join(ROOT, "scrubby_amd", "scrubby-hip")
        t0 = time.time()
        p = subprocess.run([exe, "k2-build", "-i", fa, "-o", os.path.join(a.work, "db"), "--taxid", "9606", "--name", "Homo sapiens"], capture_output=True, text=True)
        wall = time.time() - t0
        if p.returncode != 0:
            res["e2e"] = {"error": p.stderr[-500:]}
        else:
            j = json.loads(p.stdout.strip().splitlines()[-1])
            gpu_fill = j["s_fill"] + j["s_estimate"] - j["s_read"]
            res["e2e"] = dict(j, fasta_bytes=os.path.getsize(fa), fasta_write_s=round(t_write, 2), wall_s=round(wall, 2),
                              hash_k2d_bytes=os.path.getsize(os.path.join(a.work, "db", "hash.k2d")), load=round(j["size"] / j["capacity"], 4),
                              gpu_s_both_passes=round(gpu_fill, 3))
        for f in ("ref.fa", "db/hash.k2d", "db/opts.k2d", "db/taxo.k2d"):
            try:
                os.remove(os.path.join(a.work, f))
            except OSError:
                pass
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
