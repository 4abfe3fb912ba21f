"""sh_bam_filter_device (k_bam_probe, k_bam_chain, k_bam_filter) against the host mirror and the plain model on every case of
bam_util.py's table: the names, next_entry and the counts.  The names buffer lies between two 4 KiB guard bands that no call may
touch.  Only the flood may send segments to the host, and it must; the corrupt cases end with the mirror's error at the mirror's offset.
Then one run of sh_alignment_run on a .bam with SCRUBBY_HIP_GUNZIP_DEVICE=1 in a child process, against the default path."""
import os
import subprocess
import sys

import pytest

from tests import bam_util as B

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
GUARD = 4096
COUNTS = ("n_records", "n_unmapped", "n_selected", "n_cg", "n_segments", "name_bytes")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    import torch
    from scrubby_amd import lib as S
    S.require_gpu()
    seg, cap = S.bam_segment(), S.bam_segment_cap()
    cases, corrupt = B.cases(seg, cap), B.corrupt_cases(seg)
    biggest = max(len(c.text) for c in cases + corrupt)
    scanner = S.BamScanner(biggest)
    yield S, torch, scanner, cases, corrupt
    scanner.close()


class Window:
    """text[:n] in HBM behind 3 bytes of offset (the kernel's byte-wise loads) or none, and a guarded names buffer"""

    def __init__(self, S, torch, text, entry, shift=0):
        self.S, self.torch = S, torch
        self.n = len(text)
        buf = torch.full((self.n + shift + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        if self.n:
            buf[shift:shift + self.n] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
        self.d_text = buf[shift:]
        self.cap = S.bam_names_bound(self.n - entry)
        self.d_all = torch.full((self.cap + 2 * GUARD,), 0x5C, dtype=torch.uint8, device="cuda")
        self.d_names = self.d_all[GUARD:]

    def run(self, scanner, n_ref, entry, last, r, base=0):
        self.d_all.fill_(0x5C)
        names_len, nxt, st = scanner.filter_device(self.d_text, self.n, n_ref, self.d_names, entry=entry, last=last, base=base, names_cap=self.cap, **r)
        self.torch.cuda.synchronize()
        host = self.d_all.cpu().numpy()
        assert (host[:GUARD] == 0x5C).all() and (host[GUARD + self.cap:] == 0x5C).all(), "a guard band was written"
        assert (host[GUARD + names_len:GUARD + self.cap] == 0x5C).all(), "bytes behind the names were written"
        return host[GUARD:GUARD + names_len].tobytes(), nxt, st


def same_as_host(S, case, text, entry, last, r, got):
    names, nxt, st = got
    h_names, h_nxt, h_st = S.bam_filter_host(text, case.n_ref, entry=entry, last=last, **r)
    assert names == h_names and nxt == h_nxt
    for k in COUNTS:
        assert st[k] == h_st[k], k


def test_cases_match_the_mirror_and_the_model(gpu):
    S, torch, scanner, cases, _ = gpu
    for case in cases:
        w = Window(S, torch, case.text, case.first)
        for r in case.rules:
            got = w.run(scanner, case.n_ref, case.first, True, r)
            assert got[0] == B.model(case.recs, r)[0], (case.label, r)
            assert got[1] == len(case.text)
            same_as_host(S, case, case.text, case.first, True, r, got)
            st = got[2]
            assert st["n_plausible"] == int(S.bam_plausible_counts(case.text, case.n_ref).sum()), case.label
            if case.flood:
                assert st["n_fallback_segments"] > 0      # and the answer is the mirror's all the same
            else:
                assert st["n_fallback_segments"] == 0, case.label


def test_unaligned_text_and_entry_behind_the_first_record(gpu):
    S, torch, scanner, cases, _ = gpu
    for case in cases[:3]:
        w = Window(S, torch, case.text, case.first, shift=3)
        for k in (0, 1, 2):
            got = w.run(scanner, case.n_ref, case.starts[k], True, case.rules[1])
            assert got[0] == B.model(case.recs[k:], case.rules[1])[0]
            same_as_host(S, case, case.text, case.starts[k], True, case.rules[1], got)
            assert got[2]["n_fallback_segments"] == 0


def test_window_ends(gpu):
    S, torch, scanner, cases, _ = gpu
    for case in cases[:3] + [c for c in cases if c.flood]:
        r = case.rules[0]
        for label, cut, complete in B.window_cuts(case):
            text = case.text[:cut]
            k = max(i for i, s in enumerate(case.starts) if s <= cut)
            w = Window(S, torch, text, case.first)
            got = w.run(scanner, case.n_ref, case.first, False, r)
            assert got[0] == B.model(case.recs[:k], r)[0] and got[1] == case.starts[k], (case.label, label)
            same_as_host(S, case, text, case.first, False, r, got)
            if complete:
                assert w.run(scanner, case.n_ref, case.first, True, r)[0] == got[0]
            else:
                with pytest.raises(S.ScrubbyHipError, match=f"truncated BAM record at {1000 + case.starts[k]}$"):
                    w.run(scanner, case.n_ref, case.first, True, r, base=1000)
    # a window that is all tail: the entry's record is cut off
    case = cases[1]
    w = Window(S, torch, case.text[:case.starts[1] + 50], case.starts[1])
    assert w.run(scanner, case.n_ref, case.starts[1], False, case.rules[0])[:2] == (b"", case.starts[1])


def test_corrupt_records_end_with_the_mirrors_error(gpu):
    S, torch, scanner, _, corrupt = gpu
    for case in corrupt:
        with pytest.raises(S.ScrubbyHipError) as host:
            S.bam_filter_host(case.text, case.n_ref, entry=case.first, base=7 << 32, **case.rules[0])
        assert str(host.value).endswith(f"not a BAM record at {(7 << 32) + case.error_at}")
        w = Window(S, torch, case.text, case.first)
        with pytest.raises(S.ScrubbyHipError) as dev:
            w.run(scanner, case.n_ref, case.first, True, case.rules[0], base=7 << 32)
        assert str(dev.value) == str(host.value), case.label
        host_all = w.d_all.cpu().numpy()
        assert (host_all == 0x5C).all(), "an error left bytes in the names"


def test_arguments_are_refused_before_any_launch(gpu):
    S, torch, scanner, cases, _ = gpu
    case = cases[0]
    w = Window(S, torch, case.text, case.first)
    with pytest.raises(S.ScrubbyHipError, match="room for 100 name bytes"):
        scanner.filter_device(w.d_text, w.n, case.n_ref, w.d_names, entry=case.first, names_cap=100)
    small = S.BamScanner(1000)
    with pytest.raises(S.ScrubbyHipError, match="the scanner was made for 1000"):
        small.filter_device(w.d_text, w.n, case.n_ref, w.d_names, entry=case.first, names_cap=w.cap)
    small.close()


CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from scrubby_amd import lib as S
res = S.alignment_run([sys.argv[2]], [sys.argv[4]], sys.argv[3], min_len=int(sys.argv[5]), min_cov=2.0, read_ids=sys.argv[4] + ".ids")
print(json.dumps(res))
"""


def test_alignment_run_on_the_device_path(gpu, tmp_path):
    """One .bam of 6 000 records in members of 8 KiB, read with the switch on in a child process: the ids and outputs of the default path,
    every record through the kernels, no notice of a fallback."""
    import json
    recs = [B.Rec(name=b"q%d" % i, cigar=((B.M, 60 + i % 90), (B.S, 90 - i % 90)), mapq=i % 61, flag=4 if i % 17 == 0 else 0) for i in range(6000)]
    bam = tmp_path / "aln.bam"; bam.write_bytes(B.bam_file(3, recs, block=8192, level=1))
    fq = tmp_path / "r.fq"; fq.write_text("".join(f"@q{i}\nACGT\n+\nIIII\n" for i in range(0, 6000, 3)))
    out = {}
    for tag, switch in (("host", None), ("device", "1")):
        env = {k: v for k, v in os.environ.items() if k != "SCRUBBY_HIP_GUNZIP_DEVICE"}
        env["SCRUBBY_HIP_DBG_HOST"] = "1"
        if switch:
            env["SCRUBBY_HIP_GUNZIP_DEVICE"] = switch
        o = tmp_path / f"o_{tag}.fq"
        p = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(fq), str(bam), str(o), "100"], env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        out[tag] = (json.loads(p.stdout.strip().split("\n")[-1]), o.read_bytes(), open(str(o) + ".ids", "rb").read(), p.stderr)
    assert out["host"][:3] == out["device"][:3]
    exp = {r.name for r in recs if B.selects(r, B.rule(min_len=100, min_cov=2.0))}
    assert out["device"][0]["n_depleted_ids"] == len(exp) and 0 < len(exp) < 6000
    err = out["device"][3]
    assert "SCRUBBY_HIP_GUNZIP_DEVICE:" not in err, err
    assert "BAM on the device: 1 windows, 6000 records, %d selected, 0 segments walked on the host" % len(exp) in err, err
    assert "BAM on the device" not in out["host"][3]
