"""A plain `bench.py` run (no --full): exactly --steps timed steps, the headline line without the extra measurements, and
--dump-outputs writing the last step's flags - the same ones from run to run, and the ones the line counts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, capture_output=True, text=True, timeout=250)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_run_and_its_dump(tmp_path):
    d1, d2 = tmp_path / "a", tmp_path / "b"
    j = run_bench("--gpus", "1", "--small", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d1))
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["higher_is_better"] is True
    assert j["value"] == pytest.approx(200_000 / (j["ms_per_step"] * 1e-3), rel=1e-3)
    assert j["cpu_baseline"] is None and j["stratified_parity"] is None and j["host_buffer_path"] is None and j["fixed_ms_per_call"] is None
    assert "secondary" not in j
    got = {p[:-4]: np.load(d1 / p) for p in os.listdir(d1)}
    assert set(got) == {"flags", "flags_index", "flags_block_sum"}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values()) and sum(v.nbytes for v in got.values()) <= 64 << 20
    assert len(got["flags"]) == 200_000 and int((got["flags"] == 1).sum()) == j["result"]["reads_removed"]
    run_bench("--gpus", "1", "--small", "--steps", "2", "--warmup", "0", "--dump-outputs", str(d2))
    for name, v in got.items():
        assert np.array_equal(np.load(d2 / (name + ".npy")), v), name


def test_plain_run_times_exactly_its_steps(monkeypatch):
    """In process: a plain run classifies the batch --warmup + --steps times and nothing more (the small batch is one launch a step),
    and `value` is the batch over the measured time of those --steps steps."""
    import torch
    sys.path.insert(0, ROOT)
    import bench as B
    from scrubby_amd import lib as S
    calls = []
    orig = S.Context.classify

    def counted(self, *args, **kw):
        calls.append(1)
        return orig(self, *args, **kw)
    monkeypatch.setattr(S.Context, "classify", counted)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--small", "--steps", "4", "--warmup", "2"])
    a = B.parse()
    out = B.main_reads(a, 0, 1, 0, torch.device("cuda", 0), None)
    assert len(calls) == 2 + 4
    assert out["steps"] == 4 and out["value"] == pytest.approx(200_000 / (out["ms_per_step"] * 1e-3), rel=1e-3)
