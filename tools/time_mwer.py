"""Times MWER training's loss call (deepspeech/pytorch_amd/mwer.py) at the benchmark's cfg3 shape.  profiles/mwer_timing.md holds
its output.

    python tools/time_mwer.py                     # 32 clips of 12-15 s (600-751 output frames), 29 classes, references of 12 labels
                                                  # per second; nbest 4 and 8, beam widths 8 and 16

Per (nbest, beam width) it times, between device events on the launching stream, WARM warm-up calls and then CALLS timed ones:
  (a) MWERLoss: the whole from_logits call, and its stages on their own -- softmax + search + rank-major rows, error counts,
      multi-hypothesis CTC forward, weights, multi-hypothesis CTC backward;
  (b) the same rows as nbest + 1 calls of ops.ctc_loss_grad on the same logits plus the torch ops that turn their nll into the
      weights and add the weighted gradients;
  (c) the plain CTC call of the stock training step (ops.ctc_loss_grad on the references).
The logits are peaked on an alignment of each reference with noise on top, so that the n-best lists look like those of a model in
training: close to the reference and to each other, different in a few labels."""
import argparse
import json
import os
import sys
import time

WARM, CALLS = 5, 30


def _timed(fn, warm=WARM, calls=CALLS):
    import numpy as np
    import torch
    ev, wall = [], []
    for i in range(warm + calls):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        t1 = time.perf_counter()
        b.synchronize()
        if i >= warm:
            ev.append(a.elapsed_time(b) * 1e3)
            wall.append((t1 - t0) * 1e6)
    return dict(event_us_median=round(float(np.median(ev)), 1), event_us_min=round(float(np.min(ev)), 1),
                event_us_max=round(float(np.max(ev)), 1), host_us_median=round(float(np.median(wall)), 1), calls=len(ev))


def _case(peak, noise):
    """logits [T'*N][32] on the device, frame counts, flat references and their sizes (host)"""
    import numpy as np
    import torch
    rs = np.random.RandomState(0)
    N, Cc, space = 32, 29, 28
    secs = np.sort(rs.uniform(12.0, 15.0, N))[::-1]
    frames = np.minimum((secs * 50).astype(np.int64) + 1, 751)
    Tp = int(frames.max())
    logits = rs.standard_normal((Tp, N, Cc)).astype(np.float32) * noise
    refs = []
    for n in range(N):
        S = int(secs[n] * 12)
        y = rs.randint(1, space, S)
        y[5::6] = space
        for i in range(1, S):                              # no repeats: the alignment below needs no blanks between labels
            if y[i] == y[i - 1]:
                y[i] = 1 + y[i] % (space - 1)
        refs.append(y)
        pos = np.sort(rs.choice(frames[n], S, replace=False))
        path = np.zeros(frames[n], np.int64)
        for i, p in enumerate(pos):
            path[p:min(p + 2, frames[n])] = y[i]
        logits[np.arange(frames[n]), n, path] += peak
    lg = torch.zeros((Tp * N, 32), dtype=torch.float32, device="cuda")
    lg[:, :Cc] = torch.from_numpy(logits.reshape(Tp * N, Cc)).cuda()
    tsz = torch.tensor([len(r) for r in refs], dtype=torch.int32)
    return lg, torch.from_numpy(frames.astype(np.int32)).cuda(), torch.from_numpy(np.concatenate(refs).astype(np.int32)), tsz, Tp, N, Cc, space


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--peak", type=float, default=5.0)
    ap.add_argument("--noise", type=float, default=1.5)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import torch
    from deepspeech.pytorch_amd import configs, mwer, ops
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    lg, lens_dev, targets, tsz, Tp, N, Cc, space = _case(a.peak, a.noise)
    tg_dev, tsz_dev = targets.cuda(), tsz.cuda()
    offs_dev = (torch.cumsum(tsz, 0) - tsz).to(torch.int32).cuda()
    max_tl = int(tsz.max())
    print(json.dumps({"clips": N, "frames_max": Tp, "frames_min": int(lens_dev.min()), "labels_max": max_tl, "classes": Cc}), flush=True)
    plain = _timed(lambda: ops.ctc_loss_grad(lg, tg_dev, offs_dev, lens_dev, tsz_dev, Tp, N, Cc, 0, max_tl))
    print(json.dumps({"section": "(c) plain CTC: ops.ctc_loss_grad on the references", "time": plain}), flush=True)
    for K in (4, 8):
        for B in (8, 16):
            dec = BeamCTCDecoder(configs.LABELS, beam_width=B, blank_index=0)
            crit = mwer.MWERLoss(dec, nbest=K, ce_weight=0.01)
            res = {"nbest": K, "beam_width": B}
            res["(a) MWERLoss.from_logits"] = _timed(lambda: crit.from_logits(lg, targets, lens_dev, tsz, N, Tp, Cc, 0))
            last = crit.last
            res["expected_word_error_rate"] = round(crit.expected_error_rate(), 4)
            res["distinct_error_counts_per_clip_mean"] = round(float(sum(len(set(last["errors"][:, n].tolist())) for n in range(N))) / N, 2)

            def search():
                probs = ops.softmax_rows(lg, Cc).view(Tp, N, Cc).transpose(0, 1)
                return dec.nbest_device(probs, lens_dev, K)
            res["(a) softmax + search + rows"] = _timed(search)
            toks, lens = search()
            hl = lens.clamp(min=0)
            res["(a) error counts"] = _timed(lambda: ops.error_counts(toks, hl, targets, tsz, space))
            err = ops.error_counts(toks, hl, targets, tsz, space)[1]
            width = max(int(lens.max()), max_tl)
            res["longest_row"] = width
            ref_rows, ref_lens = mwer.pad_rows(targets, tsz)
            rows, all_lens = mwer.append_rank(toks, lens, torch.from_numpy(ref_rows).cuda(), torch.from_numpy(ref_lens).cuda(), width)
            fwd = lambda: ops.ctc_multi_forward(lg, rows, all_lens, lens_dev, Tp, N, Cc, 0, want_grad=True, max_target_len=width)
            res["(a) multi-CTC forward"] = _timed(fwd)
            nll, state = fwd()
            res["(a) weights"] = _timed(lambda: ops.mwer_weights(nll, err, K, True, 0.01))
            w = ops.mwer_weights(nll, err, K, True, 0.01)[0]
            res["(a) multi-CTC backward"] = _timed(lambda: ops.ctc_multi_backward(state, w, lg.shape[1]))
            res["forward-only scores of the same rows"] = _timed(
                lambda: ops.ctc_multi_forward(lg, rows, all_lens, lens_dev, Tp, N, Cc, 0, want_grad=False, max_target_len=width))
            # (b) the same rows through the single-sequence entry, one call per rank, combined with torch
            flat = [rows[r].reshape(-1) for r in range(K + 1)]
            roffs = torch.arange(N, dtype=torch.int32, device="cuda") * rows.shape[2]
            rl = [all_lens[r].clamp(min=0).contiguous() for r in range(K + 1)]
            errf = err.view(K, N).float()

            def single_calls():
                outs = [ops.ctc_loss_grad(lg, flat[r], roffs, lens_dev, rl[r], Tp, N, Cc, 0, width) for r in range(K + 1)]
                s = -torch.stack([o[1] for o in outs[:K]])
                s = torch.where(all_lens[:K] >= 0, s, torch.full_like(s, -float("inf")))
                ph = torch.softmax(s, 0)
                wk = -ph * (errf - (ph * errf).sum(0, keepdim=True))
                total = outs[K][2].view(Tp, N, -1) * 0.01
                for r in range(K):
                    total = total + outs[r][2].view(Tp, N, -1) * wk[r].view(1, N, 1)
                return total
            res["(b) nbest + 1 single calls + torch"] = _timed(single_calls)
            multi = res["(a) multi-CTC forward"]["event_us_median"] + res["(a) weights"]["event_us_median"] + res["(a) multi-CTC backward"]["event_us_median"]
            res["(b) / (a), CTC and weights only"] = round(res["(b) nbest + 1 single calls + torch"]["event_us_median"] / multi, 2)
            res["(a) whole call / (c)"] = round(res["(a) MWERLoss.from_logits"]["event_us_median"] / plain["event_us_median"], 2)
            got = ops.ctc_multi_backward(state, w, lg.shape[1]).view(Tp, N, -1)
            res["max_abs_difference_(a)_(b)"] = float((got - single_calls()).abs().max())
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
