"""Device DEFLATE alone (sh_deflate_device) on the e2e bench's FASTQ: records `@syn.<9 digits> 1:N:0:0`, 150 synthetic bases, qualities
`I` (bench.py fastq_file), --mib MiB of them resident in HBM, block 32768.  Prints one JSON line: kernel ms (stats.ms: the three kernels
between two events), GB/s of input, stored blocks, matches per KiB, and the output size beside zlib level 1 and level 6 - whole-stream,
on the CPU - over the first --zlib-mib MiB of the same bytes (the device figure for that slice is measured on that slice).

    python scripts/deflate_speed.py --mib 1024 --zlib-mib 128
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def fastq_bytes(S, n_bytes, device):
    import torch
    L = 150
    head = b"@syn.000000000 1:N:0:0\n"
    row = np.frombuffer(head + b"A" * L + b"\n+\n" + b"I" * L + b"\n", dtype=np.uint8)
    n = -(-n_bytes // row.size)
    P, R = S.ref_params(0x5C2B0001, [300_000_000]), S.read_params(0x5C2B0002)
    d_reads = torch.empty(n * L + 64, dtype=torch.uint8, device=device)
    d_off = torch.empty(n + 1, dtype=torch.int64, device=device)
    S.synth_reads_device(P, R, 0, n, d_reads, d_off)
    reads = d_reads[:n * L].cpu().numpy().reshape(n, L)
    arr = np.empty((n, row.size), dtype=np.uint8)
    arr[:] = row
    o = np.arange(n, dtype=np.int64)
    for d in range(9):
        arr[:, 5 + 8 - d] = 48 + (o % 10)
        o //= 10
    arr[:, len(head):len(head) + L] = reads
    return arr.reshape(-1)[:n_bytes]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--zlib-mib", type=int, default=128)
    ap.add_argument("--block", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    import torch
    from scrubby_amd import lib as S
    S.require_gpu()
    n = a.mib << 20
    host = fastq_bytes(S, n, "cuda")
    d_in = torch.from_numpy(host).cuda()
    d_out = torch.empty(S.deflate_bound(n, a.block), dtype=torch.uint8, device="cuda")
    df = S.Deflater(n, a.block)
    runs = []
    for _ in range(a.steps + 1):      # the first run is the warm-up
        out_len, st = df.deflate_device(d_in, n, d_out)
        runs.append(st)
    first = d_out[:out_len].cpu().numpy().tobytes()
    assert all(r["out_bytes"] == out_len for r in runs)
    ms = sorted(r["ms"] for r in runs[1:])[len(runs[1:]) // 2]
    nz = min(n, a.zlib_mib << 20)
    z_len, z_st = df.deflate_device(d_in, nz, d_out)
    sl = host[:nz].tobytes()
    assert zlib.decompress(d_out[:z_len].cpu().numpy().tobytes(), -15) == sl, "the slice does not round-trip"
    t0 = time.perf_counter(); l1 = len(zlib.compress(sl, 1)); t1 = time.perf_counter(); l6 = len(zlib.compress(sl, 6)); t2 = time.perf_counter()
    inf = zlib.decompressobj(-15)
    ok = inf.decompress(first[:64 << 20], 1 << 20) == host[:1 << 20].tobytes()      # the head of the whole stream
    st = runs[-1]
    print(json.dumps({
        "workload": f"sh_deflate_device on {a.mib} MiB of the e2e bench's FASTQ, block {a.block}", "input_bytes": n, "output_bytes": out_len,
        "ratio": round(out_len / n, 4), "ms": round(ms, 2), "ms_runs": [round(r["ms"], 2) for r in runs[1:]], "input_GB_per_s": round(n / ms / 1e6, 2),
        "n_blocks": st["n_blocks"], "n_stored": st["n_stored"], "matches_per_KiB": round(st["n_matches"] / (n / 1024), 2),
        "literals_per_KiB": round(st["n_literals"] / (n / 1024), 2), "head_round_trips": bool(ok),
        "slice": {"bytes": nz, "device": z_len, "device_ms": round(z_st["ms"], 2), "zlib_level_1": l1, "zlib_level_6": l6, "device_over_level_1": round(z_len / l1, 3),
                  "device_over_level_6": round(z_len / l6, 3), "zlib_level_1_MB_per_s_one_thread": round(nz / (t1 - t0) / 1e6, 1),
                  "zlib_level_6_MB_per_s_one_thread": round(nz / (t2 - t1) / 1e6, 1)},
    }), flush=True)


if __name__ == "__main__":
    main()
