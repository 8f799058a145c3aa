"""bench.py on the device: `--steps` sets the number of timed steps, and `--dump-outputs` writes the same files in two runs with
the same arguments (the inputs are seeded, and every reduction of cfg3's timed step adds in a fixed order)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])


def test_bench_dump_outputs_are_the_same_in_two_runs(tmp_path):
    a, b = _run(tmp_path / "a"), _run(tmp_path / "b")
    for line in (a, b):
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert line["step_time_distribution"] is not None
    names = sorted(os.listdir(tmp_path / "a"))
    assert "loss.npy" in names and any(n.startswith("grad.") for n in names) and any(n.startswith("state.") for n in names)
    assert names == sorted(os.listdir(tmp_path / "b"))
    total = 0
    for n in names:
        x, y = (tmp_path / "a" / n).read_bytes(), (tmp_path / "b" / n).read_bytes()
        assert x == y, n
        total += len(x)
    assert total <= 64 << 20
    assert a["ctc_loss_last_step"] == b["ctc_loss_last_step"]
