"""bench.py contract on CPU (tiny spec): the result line, --steps, --full (the
real ramp instead of the seeded steady state) and the reproducible
--dump-outputs arrays."""

import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPS = ("last_step_rows", "last_step_tokens", "last_step_logprobs",
         "finished_rows", "finished_tokens", "finished_logprobs",
         "step_stats")


def _run_bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
           "--steps", "3", "--warmup", "1", "--batch", "8", "--max-new", "4",
           "--prompt-len", "16", "--dump-outputs", str(out_dir), *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300,
                         cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_bench_dump_outputs_reproducible(tmp_path):
    a = _run_bench(tmp_path / "a")
    b = _run_bench(tmp_path / "b")
    full = _run_bench(tmp_path / "full", "--full")
    assert set(full) == set(a)
    for d in (a, b, full):
        assert d["metric"] == "output_tokens_per_sec"
        assert d["unit"] == "tokens/s"
        assert d["higher_is_better"] is True
        assert d["steps"] == 3 and d["warmup"] == 1
        assert d["ms_per_step"] > 0
        assert d["value"] > 0

    arrs = {}
    for name in DUMPS:
        x = np.load(tmp_path / "a" / f"{name}.npy")
        y = np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype in (np.float32, np.float64)
        assert x.shape == y.shape and np.array_equal(x, y), name
        arrs[name] = x
    assert sorted(os.listdir(tmp_path / "a")) == sorted(
        f"{n}.npy" for n in DUMPS)

    # the dump is the last step's own return: one token per row it advanced,
    # and the whole generation (at most --max-new tokens) of rows it finished
    rows, toks = arrs["last_step_rows"], arrs["last_step_tokens"]
    sched, _, n_out, n_fin = arrs["step_stats"]
    assert len(rows) == len(toks) == len(arrs["last_step_logprobs"]) == n_out
    assert 0 < n_out <= sched
    assert len(set(rows.tolist())) == len(rows)
    assert np.all(toks >= 0) and np.all(toks == np.round(toks))
    assert np.all(arrs["last_step_logprobs"] <= 0)
    assert n_fin == len(arrs["finished_rows"])
    assert n_fin == len(arrs["finished_tokens"])
    assert n_fin == len(arrs["finished_logprobs"])
    assert arrs["finished_tokens"].shape[1] <= 4
    assert set(arrs["finished_rows"].tolist()) <= set(rows.tolist())
