"""Times keyword spotting (keywords.KeywordSpotter, csrc/ds2_kws.hip) next to its yardsticks; profiles/kws_timing.md holds its output.

    python tools/time_kws.py [--output-path timing.json]        # on the GPU

One shot: ``spot`` at 32 clips x 751 frames (every second clip 600-750), C = 29, probabilities read in place as the (N, T', C)
view of the head's rows, with 1, 100 and 1000 keywords of 4-12 labels; the ds2_kws_reset + ds2_kws_feed entries alone on
preallocated buffers at the same sizes; ``GreedyDecoder.decode`` and ``ops.ctc_align`` (170-190 labels per clip) at the same shape;
the numpy restatement tests/kws_reference.py on the CPU (one clip, 100 keywords: the whole batch would take minutes).
Streamed: ``KeywordStream.feed`` of 100 streams x 8 frames with 100 and 1000 keywords against ``GreedyStream.feed`` of the same
block.  20 warm calls of every candidate, then 200 repetitions with the candidates alternating in one window, device events
around each call (they include the host's wait for the hits); median and 10th / 90th percentile.
"""
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
S, Tc = 100, 8


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


def keywords_of(rs, K, labels):
    seen = set()
    while len(seen) < K:
        seen.add(''.join(labels[i] for i in rs.randint(1, Cc, size=rs.randint(4, 13))))
    return sorted(seen)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    out_path = argv[argv.index("--output-path") + 1] if "--output-path" in argv else None
    assert torch.cuda.is_available(), "time_kws needs a HIP device"
    from deepspeech.pytorch_amd import _lib, ops
    from deepspeech.pytorch_amd.configs import LABELS
    from deepspeech.pytorch_amd.decoder import GreedyDecoder
    from deepspeech.pytorch_amd.keywords import KeywordSpotter
    import kws_reference as R

    labels = list(LABELS)[:Cc]
    rs = np.random.RandomState(0)
    sizes = np.full(N, Tp)
    sizes[1::2] = rs.randint(600, 751, size=N // 2)
    logits = (rs.standard_normal((Tp * N, LD)) * 2).astype(np.float32)
    logits[:, Cc:] = -np.inf
    rows = torch.softmax(torch.from_numpy(logits).cuda(), -1)
    x = rows.view(Tp, N, LD)[:, :, :Cc].transpose(0, 1)          # the (N, T', C) view of the head's rows, read in place
    szd = torch.from_numpy(sizes.astype(np.int32)).cuda()
    tl = rs.randint(170, 191, size=N)
    tg = torch.from_numpy(rs.randint(1, Cc, size=int(tl.sum())).astype(np.int32)).cuda()
    tld = torch.from_numpy(tl.astype(np.int32)).cuda()
    dec = GreedyDecoder(labels)

    fns, spotters, res = {}, {}, {}
    for K in (1, 100, 1000):
        sp = spotters[K] = KeywordSpotter(labels, keywords_of(np.random.RandomState(K), K, labels))
        fns["spot_K%d" % K] = (lambda sp=sp: sp.spot(x, szd, kind="probs"))
        h = ops.kws_open(N, sp.lanes, K, sp.hold, sp.max_hits, 0, "cuda")
        ws = torch.empty(_lib.query("ds2_kws_ws_bytes", N, Tp, K, sp.max_hits), dtype=torch.uint8, device="cuda")

        def entry(h=h, ws=ws, K=K, sp=sp):
            _lib.call("ds2_kws_reset", ops.P(h.state), N, h.W, K, ops.P(None), ops.S())
            _lib.call("ds2_kws_feed", ops.P(x), x.stride(0), x.stride(1), N, Tp, Cc, 1, ops.P(szd), 0, ops.P(h.lanes), h.W, K, sp.hold,
                      sp.max_hits, ops.P(None), 1, ops.P(h.state), ops.P(h.out), ops.P(ws), ops.S())
        fns["entries_K%d" % K] = entry
        res["waves_K%d" % K] = h.W
    fns["greedy_decode"] = lambda: dec.decode(x, szd)
    fns["ops_ctc_align"] = lambda: ops.ctc_align(x, szd, tg, tld, blank=0, mode="probs", max_target_len=int(tl.max()))
    res.update(timed(fns))
    res["hits_K1000"] = sum(len(d) for d in spotters[1000].spot(x, szd, kind="probs"))

    # streamed: 100 streams x 8 frames
    block = torch.softmax(torch.from_numpy((rs.standard_normal((S, Tc, Cc)) * 2).astype(np.float32)).cuda(), -1)
    sfns = {}
    gs = dec.stream(S, "cuda")
    sfns["greedy_stream_feed"] = lambda: gs.feed(block)
    for K in (100, 1000):
        ks = spotters[K].stream(S, "cuda")
        sfns["keyword_stream_feed_K%d" % K] = (lambda ks=ks: ks.feed(block))
    res.update(timed(sfns))

    # the numpy restatement on the CPU: one clip, 100 keywords
    p0 = x[0, :sizes[0]].cpu().numpy()
    sp = spotters[100]
    t0 = time.perf_counter()
    R.spot(p0, sp.label_ids, sp.thresholds, 0, sp.hold, sp.max_hits, kind="probs")
    res["restatement_cpu_one_clip_K100_ms"] = (time.perf_counter() - t0) * 1e3

    sp = spotters[1000]
    W = sp.lanes.shape[0] // 64
    res["bytes_S100_K1000"] = dict(waves=W, state=_lib.query("ds2_kws_state_bytes", S, W, 1000),
                                   out=_lib.query("ds2_kws_out_stride", 1000, sp.max_hits) * 4 * S,
                                   ws_8_frames=_lib.query("ds2_kws_ws_bytes", S, Tc, 1000, sp.max_hits), max_hits=sp.max_hits)
    res["shape"] = dict(N=N, Tp=Tp, C=Cc, keywords="4-12 labels", kind="probs", streams=S, chunk=Tc)
    print(json.dumps(res, indent=1))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
