"""Times the device CTC beam search (ops.beam_decode) beside the greedy decoder (ops.greedy_decode) on cfg3-shaped probabilities:
N = 32 utterances of T' = 751 frames over the 29 labels, rows = softmax of scaled normals (peaky, like the model's outputs).
Each call is timed with HIP events after warm-up, median of --runs calls (the host copies of the surviving labels included).

    python tools/bench_beam.py [--runs 20] [--widths 1,10,128] [--out profiles/beam_bench.txt]
    python tools/bench_beam.py --lm tests/golden/lm/toy3.arpa [--alpha 1.0 --beta 1.0 --open]

With --lm the same widths are also timed through ops.beam_decode_lm (lexicon mode unless --open), and the one-off cost of parsing
the ARPA file and of building and uploading the two tables is reported.  To make word events happen on random rows the space
label's logit is raised (--space-boost) in both the plain and the LM run.
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--lm", default=None, help="ARPA file: also time ops.beam_decode_lm")
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--open", action="store_true", help="open mode (lexicon=False)")
    ap.add_argument("--space-boost", type=float, default=0.0)
    a = ap.parse_args()
    assert a.runs >= 10
    assert torch.cuda.is_available(), "bench_beam needs a HIP device"
    N, T, C = 32, 751, 29
    rng = np.random.default_rng(0)
    z = rng.standard_normal((N, T, C)) * a.scale
    z[:, :, C - 1] += a.space_boost                       # configs.LABELS: the space is the last label
    e = np.exp(z - z.max(-1, keepdims=True))
    probs = torch.from_numpy((e / e.sum(-1, keepdims=True)).astype(np.float32)).cuda()
    sizes = torch.full((N,), T, dtype=torch.int32)
    rows = []
    med, lo, hi = timed(lambda: ops.greedy_decode(probs, sizes, 0), a.runs)
    rows.append(dict(decoder="greedy", B=None, ms_per_batch=med, min_ms=lo, max_ms=hi, us_per_step=1e3 * med / T))
    for B in [int(w) for w in a.widths.split(",")]:
        med, lo, hi = timed(lambda: ops.beam_decode(probs, sizes, 0, B, a.top_n, 1.0), a.runs)
        rows.append(dict(decoder="beam", B=B, ms_per_batch=med, min_ms=lo, max_ms=hi, us_per_step=1e3 * med / T))
    notes = []
    if a.lm:
        from deepspeech.pytorch_amd import lm as LM
        from deepspeech.pytorch_amd.configs import LABELS
        assert len(LABELS) == C and LABELS[C - 1] == ' '
        t0 = time.perf_counter()
        model = LM.load_arpa(a.lm)
        t1 = time.perf_counter()
        wt, gt = LM.build_tables(model, LABELS, 0, C - 1)
        t2 = time.perf_counter()
        wt, gt = torch.from_numpy(wt).cuda(), torch.from_numpy(gt).cuda()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        notes.append("# lm %s: order %d, n-grams %s; parse %.2f s, table build %.2f s, upload %.3f s; word table %d slots, n-gram "
                     "table %d slots (%.1f MB); alpha %.2f beta %.2f %s mode, space boost %.1f"
                     % (a.lm, model.order, model.counts, t1 - t0, t2 - t1, t3 - t2, wt.shape[0], gt.shape[0], gt.numel() * 8 / 1e6,
                        a.alpha, a.beta, "open" if a.open else "lexicon", a.space_boost))
        for B in [int(w) for w in a.widths.split(",")]:
            med, lo, hi = timed(lambda: ops.beam_decode_lm(probs, sizes, 0, B, a.top_n, 1.0, C - 1, wt, gt, model.order, model.bos,
                                                           a.alpha, a.beta, not a.open), a.runs)
            rows.append(dict(decoder="beam+lm", B=B, ms_per_batch=med, min_ms=lo, max_ms=hi, us_per_step=1e3 * med / T))
    lines = notes + ["# tools/bench_beam.py: N=%d T'=%d C=%d cutoff_top_n=%d softmax(normal * %.1f), median of %d calls after warm-up, %s"
             % (N, T, C, a.top_n, a.scale, a.runs, torch.cuda.get_device_name(0))]
    for r in rows:
        lines.append("%-7s B=%-4s %9.3f ms/batch (min %.3f, max %.3f)  %8.2f us/step" %
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
