"""Times CTC forced alignment at the benchmark's training shape (32 clips x 751 frames, 170-190 labels, 29 classes, logits) next
to two yardsticks: the ds2_ctc_loss_grad call at the same shape and the fp64 restatement tests/ctc_align_reference.py on the CPU.
profiles/ctc_align_timing.md holds its output.

    python tools/time_ctc_align.py --build-forward-only         # wherever hipcc runs (no GPU needed): the A/B library
    python tools/time_ctc_align.py [--output-path timing.json]  # on the GPU

Rows: the whole ops.ctc_align call; the ds2_ctc_align entry alone on preallocated buffers (without the wrapper's prefix sum and
allocations); and, when the A/B library libds2hip_alignfwd.so exists (the same sources with -DDS2_ALIGN_SKIP_TRACEBACK, built by
build.build_variant, never loaded by the product), the entry without its trace-back and label-span phases -- the difference of the
last two is what those phases cost.  20 warm calls of every candidate, then 200 repetitions with the candidates alternating in one
window, device events around each call; median and 10th / 90th percentile.
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

N, Tp, Cc, LD = 32, 751, 29, 32
VARIANT = os.path.join(ROOT, "deepspeech", "pytorch_amd", "libds2hip_alignfwd.so")


def timed(fns, warm=20, reps=200):
    for f in fns.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):                     # alternate the candidates inside one window
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3)
    return {k: dict(median_us=float(np.median(v)), p10_us=float(np.percentile(v, 10)), p90_us=float(np.percentile(v, 90)), reps=len(v))
            for k, v in out.items()}


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if "--build-forward-only" in argv:
        from deepspeech.pytorch_amd import build
        print(build.build_variant("alignfwd", ["-DDS2_ALIGN_SKIP_TRACEBACK"]))
        return
    out_path = argv[argv.index("--output-path") + 1] if "--output-path" in argv else None
    assert torch.cuda.is_available(), "time_ctc_align needs a HIP device"
    from deepspeech.pytorch_amd import _lib, ops
    import ctc_align_reference as R

    rs = np.random.RandomState(0)
    tl = rs.randint(170, 191, size=N)
    sizes = np.full(N, Tp)
    sizes[1::2] = rs.randint(600, 751, size=N // 2)
    targets = rs.randint(1, Cc, size=int(tl.sum()))
    logits = (rs.standard_normal((Tp * N, LD)) * 2).astype(np.float32)
    rows = torch.from_numpy(logits).cuda()
    x = rows.view(Tp, N, LD)[:, :, :Cc].transpose(0, 1)          # the (N, T', C) view of the head's rows, read in place
    tg = torch.from_numpy(targets.astype(np.int32)).cuda()
    tld = torch.from_numpy(tl.astype(np.int32)).cuda()
    szd = torch.from_numpy(sizes.astype(np.int32)).cuda()
    offs = (torch.cumsum(tld, 0, dtype=torch.int32) - tld).contiguous()
    maxl = int(tl.max())
    fs = torch.empty((N, Tp), dtype=torch.int32, device="cuda")
    tok = torch.empty((3, len(targets)), dtype=torch.int32, device="cuda")
    sc = torch.empty(N, dtype=torch.float32, device="cuda")
    ws = torch.empty(_lib.query("ds2_ctc_align_ws_bytes", Tp, N, maxl), dtype=torch.uint8, device="cuda")

    def entry_of(fn):
        def run():
            rc = fn(ops.P(x), x.stride(0), x.stride(1), N, Tp, Cc, 0, ops.P(szd), ops.P(tg), ops.P(offs), ops.P(tld), maxl, 0, ops.P(fs),
                    ops.P(tok[0]), ops.P(tok[1]), ops.P(tok[2]), ops.P(sc), ops.P(ws), ops.S())
            assert rc == 0, rc
        return run

    def align():
        return ops.ctc_align(x, szd, tg, tld, blank=0, mode="logits", max_target_len=maxl)

    def loss():
        return ops.ctc_loss_grad(rows, tg, offs, szd, tld, Tp, N, Cc, 0, maxl)

    fns = {"ops_ctc_align": align, "ops_ctc_loss_grad": loss, "ds2_ctc_align_entry": entry_of(_lib.load().ds2_ctc_align)}
    if os.path.exists(VARIANT):
        vlib = C.CDLL(VARIANT)
        vlib.ds2_ctc_align.restype, vlib.ds2_ctc_align.argtypes = _lib.SIGNATURES["ds2_ctc_align"]
        fns["ds2_ctc_align_entry_forward_only"] = entry_of(vlib.ds2_ctc_align)
    res = timed(fns)
    # at the timed size: every path is a valid alignment of its target and scores below the loss kernel's likelihood
    fsd, _, _, _, score = align()
    _, nll, _ = loss()
    score, nll, fsd = score.cpu().numpy(), nll.cpu().numpy(), fsd.cpu().numpy()
    off, ok = 0, True
    for n in range(N):
        ok &= R.collapses_to(fsd[n, :sizes[n]], targets[off:off + tl[n]], 0) and score[n] <= -nll[n] + 1e-3
        off += tl[n]
    res["valid_paths_and_score_below_likelihood"] = bool(ok)
    lp64 = torch.log_softmax(torch.from_numpy(logits[:, :Cc]).double(), -1).numpy().reshape(Tp, N, Cc)
    cpu = []
    for _ in range(3):
        t0, off = time.perf_counter(), 0
        for n in range(N):
            R.align(lp64[:sizes[n], n], targets[off:off + tl[n]], 0)
            off += tl[n]
        cpu.append((time.perf_counter() - t0) * 1e3)
    res["restatement_fp64_cpu_ms"] = dict(median=float(np.median(cpu)), min=float(min(cpu)), max=float(max(cpu)), reps=3)
    res["shape"] = dict(N=N, Tp=Tp, C=Cc, labels="170-190", mode="logits")
    print(json.dumps(res, indent=1))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
