"""Times the device CTC beam search (ops.beam_decode) beside the greedy decoder (ops.greedy_decode) on cfg3-shaped probabilities:
N = 32 utterances of T' = 751 frames over the 29 labels, rows = softmax of scaled normals (peaky, like the model's outputs).
Each call is timed with HIP events after warm-up, median of --runs calls (the host copies of the surviving labels included).

    python tools/bench_beam.py [--runs 20] [--widths 1,10,128] [--out profiles/beam_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepspeech.pytorch_amd import ops  # noqa: E402


def timed(fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--widths", default="1,10,128")
    ap.add_argument("--top-n", type=int, default=40)
    ap.add_argument("--scale", type=float, default=3.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 10
    assert torch.cuda.is_available(), "bench_beam needs a HIP device"
    N, T, C = 32, 751, 29
    rng = np.random.default_rng(0)
    z = rng.standard_normal((N, T, C)) * a.scale
    e = np.exp(z - z.max(-1, keepdims=True))
    probs = torch.from_numpy((e / e.sum(-1, keepdims=True)).astype(np.float32)).cuda()
    sizes = torch.full((N,), T, dtype=torch.int32)
    rows = []
    med, lo, hi = timed(lambda: ops.greedy_decode(probs, sizes, 0), a.runs)
    rows.append(dict(decoder="greedy", B=None, ms_per_batch=med, min_ms=lo, max_ms=hi, us_per_step=1e3 * med / T))
    for B in [int(w) for w in a.widths.split(",")]:
        med, lo, hi = timed(lambda: ops.beam_decode(probs, sizes, 0, B, a.top_n, 1.0), a.runs)
        rows.append(dict(decoder="beam", B=B, ms_per_batch=med, min_ms=lo, max_ms=hi, us_per_step=1e3 * med / T))
    lines = ["# tools/bench_beam.py: N=%d T'=%d C=%d cutoff_top_n=%d softmax(normal * %.1f), median of %d calls after warm-up, %s"
             % (N, T, C, a.top_n, a.scale, a.runs, torch.cuda.get_device_name(0))]
    for r in rows:
        lines.append("%-6s B=%-4s %9.3f ms/batch (min %.3f, max %.3f)  %8.2f us/step" %
                     (r["decoder"], r["B"] if r["B"] else "-", r["ms_per_batch"], r["min_ms"], r["max_ms"], r["us_per_step"]))
    lines.append(json.dumps(rows))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
