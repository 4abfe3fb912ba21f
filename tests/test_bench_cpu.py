"""bench.py --dump-outputs on the host side: what a dump holds (float32 / float64 only, at most 64 MB, a fixed seeded sample above the cap,
block sums over every entry), without a GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    sys.path.insert(0, ROOT)
    import bench as B
    return B


def test_pick_is_fixed_sorted_and_capped(bench):
    assert np.array_equal(bench.dump_pick(1000, 4000), np.arange(1000))
    a, b = bench.dump_pick(50_000_000, 4_000_000), bench.dump_pick(50_000_000, 4_000_000)
    assert np.array_equal(a, b) and len(a) == 4_000_000
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 50_000_000


def test_flags_dump_of_a_large_batch(bench, tmp_path):
    import torch
    n = 10_000_123
    f = (np.random.default_rng(3).random(n) < 0.5).astype(np.uint8)
    f[::97] = 2
    bench.dump_flags(str(tmp_path), torch.from_numpy(f), cap=1_000_000)
    got = {p[:-4]: np.load(tmp_path / p) for p in os.listdir(tmp_path)}
    assert set(got) == {"flags", "flags_index", "flags_block_sum"}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    idx = got["flags_index"].astype(np.int64)
    assert len(idx) == 1_000_000 and np.array_equal(got["flags"], f[idx].astype(np.float32))
    assert len(got["flags_block_sum"]) == (n + bench.DUMP_BLOCK - 1) // bench.DUMP_BLOCK
    assert got["flags_block_sum"].sum() == f.sum(dtype=np.int64) and got["flags_block_sum"][-1] == f[-(n % bench.DUMP_BLOCK):].sum()


def test_calls_dump_keeps_every_field(bench, tmp_path):
    sys.path.insert(0, ROOT)
    from scrubby_amd import k2 as K
    res = np.zeros(5000, dtype=K.RESULT_DTYPE)
    res["taxid"][::3], res["call"][::3], res["total_kmers"][:], res["hit_groups"][::3] = 9606, 11, 232, 4
    bench.dump_calls(str(tmp_path), {k: res[k] for k in res.dtype.names})
    for name in res.dtype.names:
        v = np.load(tmp_path / (name + ".npy"))
        assert v.dtype == np.float64 and np.array_equal(v, res[name].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "pair_index.npy"), np.arange(5000, dtype=np.float64))
    assert np.load(tmp_path / "classified_block_count.npy").sum() == (res["call"] != 0).sum()


def test_job_wide_bitmap_of_uneven_shards(bench):
    """N > 1 long reads: shards of equal bases, so uneven record counts; the gathered slices unpack to the job's flags."""
    import torch
    sys.path.insert(0, ROOT)
    from scrubby_amd import dist as D
    f = (np.random.default_rng(5).random(10_007) < 0.4).astype(np.uint8)
    f[::13] = 2
    cuts = [0, 1234, 7000, 10_007]
    slice_bytes = (max(cuts[r + 1] - cuts[r] for r in range(3)) + 7) // 8
    parts = []
    for r in range(3):
        bits = D.pack_flags(torch.from_numpy(f[cuts[r]:cuts[r + 1]]))
        parts.append(torch.cat([bits, torch.zeros(slice_bytes - bits.numel(), dtype=torch.uint8)]))
    got = bench.flags_of_cuts(torch.cat(parts), slice_bytes, cuts).numpy()
    assert np.array_equal(got, (f == 1).astype(np.uint8))


def test_dump_refuses_other_types_and_oversize(bench, tmp_path):
    with pytest.raises(AssertionError):
        bench.write_dump(str(tmp_path / "a"), {"x": np.zeros(4, dtype=np.int32)})
    with pytest.raises(AssertionError):
        bench.write_dump(str(tmp_path / "b"), {"x": np.zeros((64 << 20) // 8 + 1, dtype=np.float64)})
    assert not os.path.exists(tmp_path / "b")


def test_plain_run_is_lean_by_default(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
