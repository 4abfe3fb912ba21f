"""Any gzip stream on the device (sh_gunzip_*, sh_inflate.hip) on the e2e bench's FASTQ (scripts/deflate_speed.py fastq_bytes), --mib MiB of
it compressed by zlib level 6 as ONE gzip member (what `gzip -6` writes).  Three parts, one JSON line each, also written to --out-dir as
gunzip_any_{kernel,index,e2e}.json:

  kernel  the compressed bytes resident in HBM, fed in windows of --window-mib MiB through sh_gunzip_feed_device: the five stages between
          events (find, size, markers, windows, resolve) and the wall time of the feeds, GB/s of output, against one zlib thread on the
          same file on the same box; the same for chunk_bytes of 4 / 16 / 64 / 256 KiB
  index   sh_index_build_fasta on an ordinary .fa.gz of a synthetic reference of --ref-mb Mb, SCRUBBY_HIP_GUNZIP_DEVICE unset against 2,
          same process, after one warm-up of each
  e2e     sh_reads_run on the .fastq.gz (single-end) against that reference, switch unset against 2

The yardstick of index and e2e is the parent commit with the switch unset: --parent-root names a checkout of it that has been built
(its libscrubby_hip.so in place), and a child process that imports the package from there runs the same two workloads on the same
files, three runs each after a warm-up.  This tree's switch-unset runs are NOT the parent's code - the readers of sh_codec.h and the
staging of sh_inflate.hip were touched - so they are measured beside it and `unset_inside_parent_spread` says whether their median lies
between the parent's fastest and slowest run.  One more run of e2e with SCRUBBY_HIP_DBG_HOST=1, not timed, gives the readers' own
account of where their time went (the `gunzip on the device` line).

    python scripts/gunzip_speed.py --mib 512 --ref-mb 600 --parent-root ../parent --out-dir profiles
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--child-root" in sys.argv:      # the parent's package, not this tree's
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--child-root") + 1])
sys.path.insert(0, ROOT)
from scripts.deflate_speed import fastq_bytes      # noqa: E402


def gzip_one_member(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def emit(a, name, rec):
    print(json.dumps(rec), flush=True)
    if a.out_dir:
        with open(os.path.join(a.out_dir, f"gunzip_any_{name}.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


def feed_all(S, inf, d_file, n_file, d_out, chunk, window):
    """the whole file through feeds of `window` compressed bytes -> (bytes out, stats summed, wall ms)"""
    import torch
    g = inf.gunzip_open(chunk)
    total, lo, hi, out = {}, 0, min(window, n_file), 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while True:
        last = hi == n_file
        rc, consumed, out_len, st = g.feed_device(d_file[lo:], hi - lo, last, d_out[out:])
        assert rc == 0, rc
        for k, v in st.items():
            total[k] = max(total.get(k, 0), v) if k == "n_rounds" else total.get(k, 0) + v
        lo += consumed
        out += out_len
        if last and (lo == hi or (consumed == 0 and out_len == 0)):
            break
        if not last:
            hi = min(n_file, lo + window)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    g.close()
    return out, total, ms


def part_kernel(a, S, text, file_bytes):
    import torch
    t0 = time.perf_counter()
    back = zlib.decompress(file_bytes, 31)
    zlib_s = time.perf_counter() - t0
    assert len(back) == len(text)
    del back
    window = a.window_mib << 20
    d_file = torch.frombuffer(bytearray(file_bytes), dtype=torch.uint8).cuda()
    d_out = torch.empty(len(text) + 64, dtype=torch.uint8, device="cuda")
    inf = S.Inflater(window, min(len(text), 192 << 20), 16)
    sweep = {}
    for chunk_kib in (4, 16, 64, 256):
        runs = [feed_all(S, inf, d_file, len(file_bytes), d_out, chunk_kib << 10, window) for _ in range(a.steps + 1)]      # the first run is the warm-up
        n_out, st, _ = runs[-1]
        assert n_out == len(text) and d_out[:1 << 20].cpu().numpy().tobytes() == bytes(text[:1 << 20]) and d_out[n_out - 4096:n_out].cpu().numpy().tobytes() == bytes(text[-4096:])
        ms = sorted(r[2] for r in runs[1:])[a.steps // 2]
        sweep[f"{chunk_kib} KiB"] = {
            "wall_ms": round(ms, 2), "wall_ms_runs": [round(r[2], 2) for r in runs[1:]], "output_GB_per_s": round(n_out / ms / 1e6, 3),
            "stage_ms": {k[3:]: round(st[k], 2) for k in ("ms_find", "ms_size", "ms_markers", "ms_windows", "ms_resolve")},
            "n_chunks": st["n_chunks"], "n_skipped": st["n_skipped"], "n_redone": st["n_redone"], "n_rounds_max": st["n_rounds"], "n_marker_symbols": st["n_marker_symbols"]}
    inf.close()
    best = min(sweep, key=lambda k: sweep[k]["wall_ms"])
    emit(a, "kernel", {
        "workload": f"sh_gunzip_feed_device on {a.mib} MiB of the e2e bench's FASTQ as one gzip member (zlib level 6, {len(file_bytes)} bytes), resident in HBM, "
                    f"windows of {a.window_mib} MiB",
        "device": torch.cuda.get_device_name(0), "in_bytes": len(file_bytes), "out_bytes": len(text),
        "one_zlib_thread_s": round(zlib_s, 3), "one_zlib_thread_GB_per_s": round(len(text) / zlib_s / 1e9, 3),
        "chunk_bytes_sweep": sweep, "fastest_chunk_bytes": best, "speedup_over_one_zlib_thread": round(zlib_s * 1e3 / sweep[best]["wall_ms"], 2)})


def timed(fn, env):
    """wall seconds of fn() with SCRUBBY_HIP_GUNZIP_DEVICE set to env (None: unset)"""
    if env is None:
        os.environ.pop("SCRUBBY_HIP_GUNZIP_DEVICE", None)
    else:
        os.environ["SCRUBBY_HIP_GUNZIP_DEVICE"] = env
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def runs_of(fn, env, steps):
    timed(fn, env)      # warm-up (e2e: the index of this reference is built and kept)
    secs, last = [], None
    for _ in range(steps):
        t, last = timed(fn, env)
        secs.append(t)
    return secs, last


def summary(secs):
    return {"seconds": [round(t, 3) for t in secs], "median_s": round(sorted(secs)[len(secs) // 2], 3)}


def index_and_e2e_runs(S, fa, fq, work, env, steps, tag):
    """({index seconds, info}, {e2e seconds, counts}) of this process's package with the switch at env"""
    opts = S.preset("sr")

    def build():
        idx = S.Index.build_fasta(fa, opts)
        info = {k: v for k, v in idx.info().items() if k != "build_ms"}
        idx.close()
        return info
    isecs, info = runs_of(build, env, steps)
    out = os.path.join(work, f"out_{tag}.fastq")
    esecs, res = runs_of(lambda: S.reads_run([fq], [out], fa, preset="sr", json=os.path.join(work, f"r_{tag}.json"), threads=16), env, steps)
    return {"seconds": isecs, "info": info}, {"seconds": esecs, "counts": [res["reads_in"], res["reads_out"], os.path.getsize(out)]}


def child(a):
    """the parent's package (sys.path says so) with the switch unset, on files that exist"""
    from scrubby_amd import lib as S
    S.require_gpu()
    assert os.path.abspath(S.LIB_PATH).startswith(os.path.abspath(a.child_root)), S.LIB_PATH
    with tempfile.TemporaryDirectory(prefix="scrubby_gunzip_parent_") as work:
        i, e = index_and_e2e_runs(S, a.fa, a.fq, work, None, a.steps, "parent")
    print("CHILD " + json.dumps({"index": i, "e2e": e}), flush=True)


def readers_account(S, fq, fa, work):
    """the `gunzip on the device` line of one run with the switch at 2 (file descriptor 2 is the library's)"""
    path = os.path.join(work, "dbg.err")
    os.environ["SCRUBBY_HIP_GUNZIP_DEVICE"] = "2"
    os.environ["SCRUBBY_HIP_DBG_HOST"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with open(path, "wb") as f:
        os.dup2(f.fileno(), 2)
        try:
            S.reads_run([fq], [os.path.join(work, "out_dbg.fastq")], fa, preset="sr", json=os.path.join(work, "r_dbg.json"), threads=16)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
    del os.environ["SCRUBBY_HIP_DBG_HOST"]
    lines = [ln for ln in open(path, errors="replace").read().splitlines() if "gunzip on the device" in ln]
    return lines[-1].strip() if lines else None


def part_index_and_e2e(a, S, text, fq_bytes, fasta_gz, work):
    import torch
    fa, fq = os.path.join(work, "ref.fa.gz"), os.path.join(work, "reads.fastq.gz")
    with open(fa, "wb") as f:
        f.write(fasta_gz)
    with open(fq, "wb") as f:
        f.write(fq_bytes)
    n_reads = bytes(text).count(b"\n") // 4
    got = {name: index_and_e2e_runs(S, fa, fq, work, env, a.steps, name) for name, env in (("switch_unset", None), ("switch_2", "2"))}
    parent = None
    if a.parent_root:
        os.environ.pop("SCRUBBY_HIP_GUNZIP_DEVICE", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-root", a.parent_root, "--fa", fa, "--fq", fq, "--steps", str(a.steps)], capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
        assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-2000:]
        parent = json.loads(lines[-1][6:])
    account = readers_account(S, fq, fa, work)
    for k, name in ((0, "index"), (1, "e2e")):
        key = "index" if k == 0 else "e2e"
        rec = {"workload": (f"sh_index_build_fasta on an ordinary .fa.gz of a synthetic reference of {a.ref_mb} Mb ({len(fasta_gz)} bytes compressed, one member)" if k == 0 else
                            f"sh_reads_run, single-end, {n_reads} reads of the e2e bench's FASTQ as one gzip member ({len(fq_bytes)} bytes) against that reference, plain output"),
               "device": torch.cuda.get_device_name(0), "runs": {n: summary(got[n][k]["seconds"]) for n in got}}
        if k == 1:
            for n in got:
                rec["runs"][n]["M_reads_per_s"] = round(n_reads / rec["runs"][n]["median_s"] / 1e6, 2)
            rec["same_counts_and_output_size"] = got["switch_unset"][1]["counts"] == got["switch_2"][1]["counts"]
            rec["readers_account_switch_2"] = account
        else:
            rec["same_index"] = got["switch_unset"][0]["info"] == got["switch_2"][0]["info"]
        if parent:
            ps = parent[key]["seconds"]
            rec["runs"]["parent_switch_unset"] = summary(ps)
            rec["unset_inside_parent_spread"] = min(ps) <= sorted(got["switch_unset"][k]["seconds"])[a.steps // 2] <= max(ps)
            rec["speedup_over_parent"] = round(rec["runs"]["parent_switch_unset"]["median_s"] / rec["runs"]["switch_2"]["median_s"], 2)
        rec["speedup"] = round(rec["runs"]["switch_unset"]["median_s"] / rec["runs"]["switch_2"]["median_s"], 2)
        emit(a, name, rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=512)
    ap.add_argument("--ref-mb", type=int, default=600)
    ap.add_argument("--window-mib", type=int, default=32)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--parts", default="kernel,index,e2e")
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its switch-unset runs are the yardstick")
    ap.add_argument("--child-root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--fa", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--fq", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_root:
        return child(a)
    import torch
    from scrubby_amd import lib as S
    S.require_gpu()
    text = fastq_bytes(S, a.mib << 20, "cuda")
    text = text[:len(text) - len(text) % 327]      # whole records: 23 bytes of header, 150 bases, `\n+\n`, 150 qualities, `\n`
    parts = a.parts.split(",")
    fasta = None
    if "index" in parts or "e2e" in parts:
        contigs = [a.ref_mb * 1_000_000 // 4] * 4
        P = S.ref_params(0x5C2B0001, contigs)
        d_ref = torch.empty(P.genome_len + 64, dtype=torch.uint8, device="cuda")
        S.synth_ref_device(P, 0, P.genome_len, d_ref)
        h_ref = d_ref[:P.genome_len].cpu().numpy()
        del d_ref
        fasta = b"".join(b">ctg%d synthetic\n" % i + h_ref[P.contig_start[i]:P.contig_start[i + 1]].tobytes() + b"\n" for i in range(len(contigs)))
    with ThreadPoolExecutor(2) as ex:      # each file is ONE member, so one zlib thread each; zlib releases the interpreter lock
        f1 = ex.submit(gzip_one_member, bytes(text))
        f2 = ex.submit(gzip_one_member, fasta) if fasta is not None else None
        file_bytes, fasta_gz = f1.result(), f2.result() if f2 else None
    if "kernel" in parts:
        part_kernel(a, S, text, file_bytes)
    if fasta_gz is not None:
        with tempfile.TemporaryDirectory(prefix="scrubby_gunzip_any_") as work:
            part_index_and_e2e(a, S, text, file_bytes, fasta_gz, work)


if __name__ == "__main__":
    main()
