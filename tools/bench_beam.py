"""Times the device CTC beam search (ops.beam_decode) beside the greedy decoder (ops.greedy_decode) on cfg3-shaped probabilities:
N = 32 utterances of T' = 751 frames over the 29 labels, rows = softmax of scaled normals (peaky, like the model's outputs).
Each call is timed with HIP events after warm-up, median of --runs calls (the host copies of the surviving labels included).

    python tools/bench_beam.py [--runs 20] [--widths 1,10,128] [--out profiles/beam_bench.txt]
    python tools/bench_beam.py --lm tests/golden/lm/toy3.arpa [--alpha 1.0 --beta 1.0 --open]

With --lm the same widths are also timed through ops.beam_decode_lm (lexicon mode unless --open), and the one-off cost of parsing
the ARPA file and of building and uploading the two tables is reported.  To make word events happen on random rows the space
label's logit is raised (--space-boost) in both the plain and the LM run.

    python tools/bench_beam.py --lm tests/golden/lm/toy3.arpa --grid 1,8,64 [--widths 10,128]

With --grid the weight search is timed at G points: one ops.beam_decode_lm_grid call plus ops.error_counts ("grid"), against G
sequential ops.beam_decode_lm calls, each followed by the host metrics on the best transcripts ("loop", the path without the grid
entry).  Both are reported as the whole call and as its device kernels alone (the raw entries on a preallocated workspace).

    python tools/bench_beam.py --stream 100 [--lm tests/golden/lm/toy3.arpa] [--widths 10,128]

With --stream the resumable search (ops.beam_stream_*) is timed per width on the same input cut into chunks of that many frames:
the one-shot call, the sum of the chunked feeds with one result fetch at the end, a single feed without and with the result fetch,
and the first feed of a stream against the feed of its last CHUNK_FRAMES frames: the same chunk length, so the two differ only
in the frames already consumed (the state is put back before every repetition, outside the timed interval).  The last of the
chunked feeds is shorter where CHUNK_FRAMES does not divide T'; it is not the "last feed" that is timed on its own.

    python tools/bench_beam.py --hot 100 [--lm tests/golden/lm/toy3.arpa] [--stream 100]

    python tools/bench_beam.py --lm tests/golden/lm/char3.arpa --lm-unit char --space-token "|" [--grid 16] [--stream 100]
    python tools/bench_beam.py --lm tests/golden/lm/cjk3.arpa --lm-unit char --top-n 64

With --lm-unit char the file is a character model and the widths are timed through ops.beam_decode_clm ("beam+clm"), the grid
through ops.beam_decode_clm_grid and the stream through ds2_beam_stream_feed_clm.  A file whose unigrams are not all English
labels (the CJK fixture) gets an input with one class per unigram besides the blank.

With --hot the same widths are also timed through ops.beam_decode_hot (and, with --lm, ops.beam_decode_lm_hot; with --stream the
hot streams too) on N synthetic phrases: half of them words cut from the input's own greedy transcripts, so that matches start,
run on and complete, the other half random letter strings of one or two words.

    python tools/bench_beam.py --words [--widths 1,10,128]

With --words the word timings and confidences are timed per width: decoder.decode_words at nbest = 1 and nbest = B against
decode_beams on the same input, the confidence pass alone on hypotheses that are already on the device (ops.confidence: both
kernels, and the same call on hypotheses of length 0, which leaves the frame kernel), and a BeamStream's best_words() against
its best() after the whole input was fed.
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


def timed(fn, runs, warmup=3, prep=None):
    """median, min and max of fn's time over runs calls after warm-up; prep() runs before every call, outside the timed interval"""
    for _ in range(warmup):
        if prep:
            prep()
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        if prep:
            prep()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def hot_phrases(probs, sizes, count, labels, seed=2):
    """count phrases (weight 2.0 per label): half of them words of the input's greedy transcripts, half random letter strings"""
    rng = np.random.default_rng(seed)
    toks, _ = ops.greedy_decode(probs, sizes, 0)
    words = sorted({w for t in toks for w in ''.join(labels[v] for v in t).split(' ') if 2 <= len(w) <= 8})
    rng.shuffle(words)
    letters = [c for c in labels[1:] if c != ' ']
    out = list(words[:count // 2])
    while len(out) < count:
        w = ' '.join(''.join(rng.choice(letters, size=int(rng.integers(3, 9)))) for _ in range(int(rng.integers(1, 3))))
        # no duplicate, and no phrase that followed by a space starts another (hotwords.py refuses both)
        if w not in out and not any(o.startswith(w + ' ') or w.startswith(o + ' ') for o in out):
            out.append(w)
    return out


def stream_rows(a, probs, lm, oneshot, hot=None):
    """the resumable search against the one-shot call oneshot(B), per width; lm / hot: None or ops.beam_stream_open's dicts"""
    N, T, C = probs.shape
    Tc = a.stream
    assert 1 <= Tc <= T
    chunks = [probs[:, i:i + Tc] for i in range(0, T, Tc)]
    rows = []
    for B in [int(w) for w in a.widths.split(",")]:
        h = ops.beam_stream_open(N, T, C, 0, B, a.top_n, 1.0, "cuda", lm, hot)
        states = h.state[:h.N * h.state_stride]          # what a feed reads and writes besides the pool slots of its own frames

        def chunked():
            ops.beam_stream_reset(h)
            for c in chunks:
                ops.beam_stream_feed(h, c)
            return ops.beam_stream_result(h, T)

        ops.beam_stream_reset(h)
        for i in range(0, T - Tc, Tc):                   # everything but the last Tc frames (the last of these feeds may overlap
            c = probs[:, i:min(i + Tc, T - Tc)]          # nothing: it is cut at T - Tc)
            ops.beam_stream_feed(h, c)
        late = states.clone()
        fresh = lambda: ops.beam_stream_reset(h)
        resume = lambda: states.copy_(late)
        row = dict(decoder="stream" + (("+clm" if lm.get("unit") == "char" else "+lm") if lm else "") + ("+hot" if hot else ""), B=B, chunk=Tc, feeds=len(chunks))
        row["oneshot_ms"], row["oneshot_min"], row["oneshot_max"] = timed(lambda: oneshot(B), a.runs)
        row["chunked_ms"], row["chunked_min"], row["chunked_max"] = timed(chunked, a.runs)
        row["feed_ms"], row["feed_min"], row["feed_max"] = timed(lambda: ops.beam_stream_feed(h, chunks[0]), a.runs, prep=fresh)
        row["feed_result_ms"], row["feed_result_min"], row["feed_result_max"] = \
            timed(lambda: ops.beam_stream_feed(h, chunks[0], row_stride=Tc), a.runs, prep=fresh)
        row["first_ms"], row["first_min"], row["first_max"] = row["feed_ms"], row["feed_min"], row["feed_max"]
        row["last_ms"], row["last_min"], row["last_max"] = \
            timed(lambda: ops.beam_stream_feed(h, probs[:, T - Tc:]), a.runs, prep=resume)
        if a.endpoint:
            row.update(endpoint_fields(a, h, chunks[0]))
        rows.append(row)
    return rows


def endpoint_fields(a, h, chunk):
    """--endpoint: the feed of frames 0..chunk through the endpointers (decoder.Endpointer's default rule; the chunk goes in
    sub-feeds of min_trailing frames as EndpointedBeamStream feeds it), and its launches timed apart for one sub-feed: the
    endpoint kernel, the search with and without the output stage, and the second pass over the frames after a cut"""
    mt, ml, ms = 50, 250, min(1000, h.max_frames)
    eh = ops.endpoint_open(h.N, 0, 0.8, mt, ml, ms)
    sink = ops.endpoint_sink_open(h, 1, ms, 8)
    L = min(mt, ml, ms)
    sub = chunk[:, :L]
    zero = torch.zeros(h.N, dtype=torch.int32, device=chunk.device)

    def fresh():
        ops.beam_stream_reset(h)
        ops.endpoint_reset(eh)
        sink.pending.zero_()

    def feed():
        for i in range(0, chunk.shape[1], L):
            ops.endpoint_beam_feed(eh, h, sink, chunk[:, i:i + L])

    def second_pass():
        y = ops.endpoint_gather(sub, zero, zero)
        ops.endpoint_feed(eh, y, zero)
        ops.beam_stream_feed(h, y, zero)

    none = torch.zeros((4, h.N), dtype=torch.int32, device=chunk.device)       # an event block in which no stream ended

    def commit_reset():
        ops._endpoint_commit(none, sink)
        ops.call("ds2_beam_stream_reset", ops.P(h.state), h.N, h.B, h.max_frames, h.flags, ops.P(none[0]), ops.S())

    out = {}
    for key, fn in (("ep_feed", feed), ("ep_detect", lambda: ops.endpoint_feed(eh, sub)), ("ep_search", lambda: ops.beam_stream_feed(h, sub)),
                    ("ep_search_out", lambda: ops._beam_stream_launch(h, sub, L, None, sink.buf, sink.lens, sink.scores, ms, 1)),
                    ("ep_commit_reset", commit_reset),
                    ("ep_second_pass", second_pass)):
        out[key + "_ms"], out[key + "_min"], out[key + "_max"] = timed(fn, a.runs, prep=fresh)
    out["ep_sub_feeds"], out["ep_sub_frames"] = -(-chunk.shape[1] // L), L
    out["ep_bytes_per_stream"] = (h.state.numel() + sink.ring.numel() * 4 + sink.buf.numel() * 4) // h.N
    return out


def grid_rows(a, probs, sizes, wt, gt, model, C):
    """the weight search at G points: the grid entry + error_counts against G single-point calls + the host metrics"""
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.configs import LABELS
    from deepspeech.pytorch_amd.ops import P, S, call, query
    N, T, _ = probs.shape
    rng = np.random.default_rng(1)
    tsz = rng.integers(60, 140, size=N)
    targets = torch.from_numpy(rng.integers(1, C, size=int(tsz.sum())).astype(np.int32))
    tsz = torch.from_numpy(tsz.astype(np.int32))
    tgt_strings = D.GreedyDecoder(LABELS).convert_to_strings(list(torch.split(targets, tsz.tolist())))
    sz = sizes.cuda()
    rows = []
    for B in [int(w) for w in a.widths.split(",")]:
        for G in [int(g) for g in a.grid.split(",")]:
            al = np.linspace(0.0, 2.0, G).astype(np.float32)
            be = np.linspace(2.0, 0.0, G).astype(np.float32)
            lm_args = (0, B, a.top_n, 1.0, C - 1, wt, gt, model.order, model.bos)

            def grid_call():
                toks, _, lens, _, _ = ops.beam_decode_lm_grid(probs, sizes, *lm_args, al, be, not a.open)
                return ops.error_counts(toks, lens, targets, tsz, C - 1)

            def loop_call():
                for g in range(G):
                    toks, _, _, _ = ops.beam_decode_lm(probs, sizes, *lm_args, float(al[g]), float(be[g]), not a.open)
                    wer, cer = D.WordErrorRate(None, None), D.CharErrorRate(None, None)
                    for n in range(N):
                        hyp = ''.join(LABELS[v] for v in toks[n][0])
                        wer.calculate_metric(hyp, tgt_strings[n][0])
                        cer.calculate_metric(hyp, tgt_strings[n][0])

            # the kernels alone: raw entries, everything allocated beforehand
            ws = torch.empty(query("ds2_beam_grid_ws_bytes", G, N, T, B), dtype=torch.uint8, device="cuda")
            gbuf = torch.zeros((2, G, N, T), dtype=torch.int32, device="cuda")
            glen = torch.zeros((G, N), dtype=torch.int32, device="cuda")
            gsc = torch.zeros((2, G, N), dtype=torch.float32, device="cuda")
            bbuf = torch.zeros((2, N, B, T), dtype=torch.int32, device="cuda")
            blen = torch.zeros((N, B), dtype=torch.int32, device="cuda")
            bsc = torch.zeros((2, N, B), dtype=torch.float32, device="cuda")
            ald, bed = torch.from_numpy(al).cuda(), torch.from_numpy(be).cuda()
            tg = targets.cuda()
            offs = torch.zeros(N + 1, dtype=torch.int32, device="cuda")
            offs[1:] = torch.cumsum(tsz.cuda(), 0)
            cnt = torch.zeros(2 * G * N + 2 * N, dtype=torch.int32, device="cuda")
            head = (P(probs), probs.stride(0), probs.stride(1), N, T, C, P(sz), 0, B, a.top_n, 1.0, C - 1, P(wt), wt.shape[0], P(gt),
                    gt.shape[0], model.order, model.bos)

            def grid_kernels():
                call("ds2_beam_decode_lm_grid", *head, int(not a.open), G, P(ald), P(bed), P(gbuf[0]), P(gbuf[1]), P(glen), P(gsc[0]),
                     P(gsc[1]), P(ws), S())
                call("ds2_error_counts", P(gbuf[0]), T, P(glen), G * N, P(tg), P(offs), N, C - 1, P(cnt[:G * N]), P(cnt[G * N:]),
                     P(cnt[2 * G * N:]), P(cnt[2 * G * N + N:]), S())

            def loop_kernels():
                for g in range(G):
                    call("ds2_beam_decode_lm", *head, float(al[g]), float(be[g]), int(not a.open), P(bbuf[0]), P(bbuf[1]), P(blen),
                         P(bsc[0]), P(bsc[1]), P(ws), S())

            for name, whole, kernels in (("grid", grid_call, grid_kernels), ("loop", loop_call, loop_kernels)):
                med, lo, hi = timed(whole, a.runs, warmup=2)
                kmed, _, _ = timed(kernels, a.runs, warmup=2)
                rows.append(dict(decoder=name, B=B, G=G, ms_per_call=med, min_ms=lo, max_ms=hi, kernel_ms=kmed, ms_per_point=med / G))
    return rows


def char_lm_rows(a, probs, sizes, model, labels):
    """--lm-unit char: ops.beam_decode_clm per width; with --grid the grid entry against a loop of single-point calls (the
    ops calls, and the raw entries on buffers allocated beforehand); with --stream the resumable search.  Returns (rows, note)."""
    from deepspeech.pytorch_amd import lm as LM
    from deepspeech.pytorch_amd.ops import P, S, call, query
    N, T, C = probs.shape
    t0 = time.perf_counter()
    ids, gt = LM.build_char_tables(model, labels, 0, a.space_token, a.table_spread or LM.CHAR_TABLE_SPREAD)
    t1 = time.perf_counter()
    ids, gt = torch.from_numpy(ids).cuda(), torch.from_numpy(gt).cuda()
    note = ("# character lm %s: order %d, n-grams %s; %d of %d labels have a unigram, space token %r; table build %.2f s, n-gram "
            "table %d slots (%.1f KB); alpha %.2f beta %.2f"
            % (a.lm, model.order, model.counts, int((ids >= 0).sum()), C - 1, a.space_token, t1 - t0, gt.shape[0], gt.numel() * 8 / 1e3,
               a.alpha, a.beta))
    rows = []
    tail = (ids, gt, model.order, model.bos)
    for B in [int(w) for w in a.widths.split(",")]:
        med, lo, hi = timed(lambda: ops.beam_decode_clm(probs, sizes, 0, B, a.top_n, 1.0, *tail, a.alpha, a.beta), a.runs)
        rows.append(dict(decoder="beam+clm", B=B, ms_per_batch=med, min_ms=lo, max_ms=hi, us_per_step=1e3 * med / T))
    sz = sizes.cuda()
    for B in [int(w) for w in a.widths.split(",")] if a.grid else []:
        for G in [int(g) for g in a.grid.split(",")]:
            al = np.linspace(0.0, 2.0, G).astype(np.float32)
            be = np.linspace(2.0, 0.0, G).astype(np.float32)
            ws = torch.empty(query("ds2_beam_grid_ws_bytes", G, N, T, B), dtype=torch.uint8, device="cuda")
            gbuf = torch.zeros((2, G, N, T), dtype=torch.int32, device="cuda")
            glen = torch.zeros((G, N), dtype=torch.int32, device="cuda")
            gsc = torch.zeros((2, G, N), dtype=torch.float32, device="cuda")
            bbuf = torch.zeros((2, N, B, T), dtype=torch.int32, device="cuda")
            blen = torch.zeros((N, B), dtype=torch.int32, device="cuda")
            bsc = torch.zeros((2, N, B), dtype=torch.float32, device="cuda")
            ald, bed = torch.from_numpy(al).cuda(), torch.from_numpy(be).cuda()
            head = (P(probs), probs.stride(0), probs.stride(1), N, T, C, P(sz), 0, B, a.top_n, 1.0, P(ids), P(gt), gt.shape[0],
                    model.order, model.bos)

            def grid_kernels():
                call("ds2_beam_decode_clm_grid", *head, G, P(ald), P(bed), P(gbuf[0]), P(gbuf[1]), P(glen), P(gsc[0]), P(gsc[1]),
                     P(ws), S())

            def loop_kernels():
                for g in range(G):
                    call("ds2_beam_decode_clm", *head, float(al[g]), float(be[g]), P(bbuf[0]), P(bbuf[1]), P(blen), P(bsc[0]),
                         P(bsc[1]), P(ws), S())

            def loop_call():
                for g in range(G):
                    ops.beam_decode_clm(probs, sizes, 0, B, a.top_n, 1.0, *tail, float(al[g]), float(be[g]))

            for name, whole, kernels in (("grid", lambda: ops.beam_decode_clm_grid(probs, sizes, 0, B, a.top_n, 1.0, *tail, al, be),
                                          grid_kernels), ("loop", loop_call, loop_kernels)):
                med, lo, hi = timed(whole, a.runs, warmup=2)
                kmed, _, _ = timed(kernels, a.runs, warmup=2)
                rows.append(dict(decoder=name, B=B, G=G, ms_per_call=med, min_ms=lo, max_ms=hi, kernel_ms=kmed, ms_per_point=med / G))
    if a.stream:
        lm_args = dict(unit="char", label_ids=ids, ngram_table=gt, order=model.order, bos=model.bos, alpha=a.alpha, beta=a.beta)
        rows += stream_rows(a, probs, lm_args, lambda B: ops.beam_decode_clm(probs, sizes, 0, B, a.top_n, 1.0, *tail, a.alpha, a.beta))
    return rows, note


def words_rows(a, probs, sizes):
    """decode_words against decode_beams, the confidence pass alone, and the streamed best_words() against best(), per width"""
    from deepspeech.pytorch_amd.configs import LABELS
    from deepspeech.pytorch_amd.confidence import Confidence
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder, GreedyDecoder
    N, T, C = probs.shape
    conf, rows = Confidence(), []
    g = GreedyDecoder(LABELS)
    row = dict(decoder="words", B=0)
    row["beams_ms"], _, _ = timed(lambda: g.decode(probs, sizes), a.runs)
    row["words1_ms"], _, _ = timed(lambda: g.decode_words(probs, sizes, conf), a.runs)
    rows.append(row)
    for B in [int(w) for w in a.widths.split(",")]:
        d = BeamCTCDecoder(LABELS, beam_width=B, cutoff_top_n=a.top_n)
        row = dict(decoder="words", B=B)
        row["beams_ms"], _, _ = timed(lambda: d.decode_beams(probs, sizes), a.runs)
        row["words1_ms"], _, _ = timed(lambda: d.decode_words(probs, sizes, conf, nbest=1), a.runs)
        row["wordsB_ms"], _, _ = timed(lambda: d.decode_words(probs, sizes, conf, nbest=B), a.runs)
        toks, offs, _ = ops.beam_decode(probs, sizes, 0, B, a.top_n, 1.0)
        tk = torch.zeros((N, B, T), dtype=torch.int32)
        of, ln = torch.zeros_like(tk), torch.zeros((N, B), dtype=torch.int32)
        for n in range(N):
            for b in range(B):
                L = len(toks[n][b])
                tk[n, b, :L], of[n, b, :L], ln[n, b] = torch.tensor(toks[n][b], dtype=torch.int32), offs[n][b], L
        tk, of, ln = tk.cuda(), of.cuda(), ln.cuda()
        for name, measure in (("pass", "label_prob"), ("pass_entropy", "entropy")):
            row[name + "_ms"], _, _ = timed(lambda: ops.confidence(probs, sizes, tk, of, ln, 0, C - 1, measure), a.runs)
            row[name + "_frames_ms"], _, _ = timed(lambda: ops.confidence(probs, sizes, tk, of, torch.zeros_like(ln), 0, C - 1, measure),
                                                   a.runs)
        row["pass1_ms"], _, _ = timed(lambda: ops.confidence(probs, sizes, tk[:, :1], of[:, :1], ln[:, :1], 0, C - 1), a.runs)
        row["mean_len"] = float(ln.float().mean())
        for name, c in (("stream", None), ("stream_conf", conf)):
            st = d.stream(N, T, "cuda", confidence=c)
            st.feed(probs, sizes.tolist())
            row[name + "_best_ms"], _, _ = timed(st.best, a.runs)
            if c is not None:
                row["stream_best_words_ms"], _, _ = timed(st.best_words, a.runs)
                row["stream_feed_conf_ms"], _, _ = timed(lambda: st.feed(probs, sizes.tolist()), a.runs, prep=st.reset)
            else:
                row["stream_feed_ms"], _, _ = timed(lambda: st.feed(probs, sizes.tolist()), a.runs, prep=st.reset)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--widths", default="1,10,128")
    ap.add_argument("--top-n", type=int, default=40)
    ap.add_argument("--scale", type=float, default=3.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lm", default=None, help="ARPA file: also time ops.beam_decode_lm")
    ap.add_argument("--lm-unit", default="word", choices=["word", "char"],
                    help="char: the file is a character model, timed through ops.beam_decode_clm (with --grid and --stream too); "
                         "when its unigrams are not all English labels the input has one class per unigram and the blank")
    ap.add_argument("--space-token", default=None, help="with --lm-unit char: the unigram that stands for the space label")
    ap.add_argument("--table-spread", type=int, default=None,
                    help="with --lm-unit char: slots of the n-gram table as a multiple of the word mode's (default: lm.CHAR_TABLE_SPREAD)")
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--open", action="store_true", help="open mode (lexicon=False)")
    ap.add_argument("--space-boost", type=float, default=0.0)
    ap.add_argument("--grid", default=None, help="with --lm: numbers of (alpha, beta) points, e.g. 1,8,64")
    ap.add_argument("--hot", type=int, default=0, metavar="N", help="also time the hot-word entries on N synthetic phrases")
    ap.add_argument("--hot-oov-logp", type=float, default=-11.5)
    ap.add_argument("--stream", type=int, default=None, metavar="CHUNK_FRAMES", help="also time the resumable search in chunks")
    ap.add_argument("--endpoint", action="store_true", help="with --stream: also time the feed with endpointing (DESIGN.md 3.6.5)")
    ap.add_argument("--words", action="store_true", help="also time decode_words and the confidence pass (DESIGN.md 3.8)")
    a = ap.parse_args()
    assert a.runs >= 10
    assert torch.cuda.is_available(), "bench_beam needs a HIP device"
    N, T, C = 32, 751, 29
    char_model = char_labels = None
    if a.lm and a.lm_unit == "char":
        from deepspeech.pytorch_amd import lm as LM
        from deepspeech.pytorch_amd.configs import LABELS
        char_model, char_labels = LM.load_arpa(a.lm), list(LABELS)
        units = [w for w in char_model.words if w not in LM.SPECIAL_TOKENS]
        if not all(w in LABELS or w == a.space_token for w in units):
            char_labels = ["_"] + units                   # a label set of the file's own, e.g. the CJK fixture: no space
            C = len(char_labels)
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
    ht = None
    if a.hot:
        from deepspeech.pytorch_amd import hotwords as HW
        from deepspeech.pytorch_amd.configs import LABELS
        assert len(LABELS) == C and LABELS[C - 1] == ' '
        phrases = hot_phrases(probs, sizes, a.hot, LABELS)
        t0 = time.perf_counter()
        table = HW.build_table(phrases, LABELS, 0, 2.0)
        t1 = time.perf_counter()
        ht = torch.from_numpy(table).cuda()
        notes.append("# hot words: %d phrases (%d from the input's greedy transcripts), weight 2.0 per label; table build %.3f s, %d "
                     "slots (%.1f KB)" % (len(phrases), a.hot // 2, t1 - t0, ht.shape[0], ht.numel() * 8 / 1e3))
        for B in [int(w) for w in a.widths.split(",")]:
            med, lo, hi = timed(lambda: ops.beam_decode_hot(probs, sizes, 0, B, a.top_n, 1.0, C - 1, ht), a.runs)
            rows.append(dict(decoder="beam+hot", B=B, ms_per_batch=med, min_ms=lo, max_ms=hi, us_per_step=1e3 * med / T))
    if char_model is not None:
        more, note = char_lm_rows(a, probs, sizes, char_model, char_labels)
        rows += more
        notes.append(note)
    elif a.lm:
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
            if ht is not None:
                med, lo, hi = timed(lambda: ops.beam_decode_lm_hot(probs, sizes, 0, B, a.top_n, 1.0, C - 1, wt, gt, model.order,
                                                                   model.bos, a.alpha, a.beta, not a.open, ht, a.hot_oov_logp), a.runs)
                rows.append(dict(decoder="beam+lm+hot", B=B, ms_per_batch=med, min_ms=lo, max_ms=hi, us_per_step=1e3 * med / T))
    if a.lm and a.grid and char_model is None:
        rows += grid_rows(a, probs, sizes, wt, gt, model, C)
    if a.stream:
        rows += stream_rows(a, probs, None, lambda B: ops.beam_decode(probs, sizes, 0, B, a.top_n, 1.0))
        hot_args = None if ht is None else dict(space=C - 1, table=ht, oov_logp=a.hot_oov_logp)
        if ht is not None:
            rows += stream_rows(a, probs, None, lambda B: ops.beam_decode_hot(probs, sizes, 0, B, a.top_n, 1.0, C - 1, ht), hot_args)
        if a.lm and char_model is None:
            lm_args = dict(space=C - 1, word_table=wt, ngram_table=gt, order=model.order, bos=model.bos, alpha=a.alpha, beta=a.beta,
                           lexicon=not a.open)
            rows += stream_rows(a, probs, lm_args,
                                lambda B: ops.beam_decode_lm(probs, sizes, 0, B, a.top_n, 1.0, C - 1, wt, gt, model.order, model.bos,
                                                             a.alpha, a.beta, not a.open))
            if ht is not None:
                rows += stream_rows(a, probs, lm_args,
                                    lambda B: ops.beam_decode_lm_hot(probs, sizes, 0, B, a.top_n, 1.0, C - 1, wt, gt, model.order,
                                                                     model.bos, a.alpha, a.beta, not a.open, ht, a.hot_oov_logp),
                                    hot_args)
    if a.words:
        rows += words_rows(a, probs, sizes)
    lines = notes + ["# tools/bench_beam.py: N=%d T'=%d C=%d cutoff_top_n=%d softmax(normal * %.1f), median of %d calls after warm-up, %s"
             % (N, T, C, a.top_n, a.scale, a.runs, torch.cuda.get_device_name(0))]
    for r in rows:
        if r["decoder"].startswith("stream"):
            lines.append("%-13s B=%-4d chunk=%-4d one-shot %8.3f ms (min %.3f, max %.3f) | %d feeds + result %8.3f ms (min %.3f, max %.3f) | "
                         "feed of frames 0..chunk %.3f ms, the same + result %.3f ms | feed of the first chunk frames %.3f ms (min %.3f, "
                         "max %.3f), of the last chunk frames (T'-chunk..T') %.3f ms (min %.3f, max %.3f)" % (r["decoder"], r["B"], r["chunk"], r["oneshot_ms"], r["oneshot_min"], r["oneshot_max"], r["feeds"],
                                        r["chunked_ms"], r["chunked_min"], r["chunked_max"], r["feed_ms"], r["feed_result_ms"],
                                        r["first_ms"], r["first_min"], r["first_max"], r["last_ms"], r["last_min"], r["last_max"]))
            if "ep_feed_ms" in r:
                lines.append("%-13s B=%-4d chunk=%-4d endpointed feed of frames 0..chunk (%d sub-feeds of <= %d frames) %.3f ms (min %.3f, "
                             "max %.3f) | one sub-feed's launches apart: endpoint kernel %.3f ms, search %.3f ms, search + output stage "
                             "%.3f ms, commit + masked reset %.3f ms, second pass (gather, endpoint kernel, search; nothing after the "
                             "cut) %.3f ms | %d bytes per stream" % (r["decoder"], r["B"], r["chunk"], r["ep_sub_feeds"], r["ep_sub_frames"],
                                                                     r["ep_feed_ms"], r["ep_feed_min"], r["ep_feed_max"], r["ep_detect_ms"],
                                                                     r["ep_search_ms"], r["ep_search_out_ms"], r["ep_commit_reset_ms"],
                                                                     r["ep_second_pass_ms"], r["ep_bytes_per_stream"]))
            continue
        if r["decoder"] == "words" and r["B"] == 0:
            lines.append("words greedy   decode %8.3f ms | decode_words %8.3f ms" % (r["beams_ms"], r["words1_ms"]))
            continue
        if r["decoder"] == "words":
            lines.append("words B=%-4d    decode_beams %8.3f ms | decode_words nbest=1 %8.3f ms, nbest=B %8.3f ms | the pass alone on B "
                         "hypotheses of %.0f labels on average: label_prob %.3f ms (frame kernel alone %.3f), entropy %.3f ms (frame "
                         "kernel alone %.3f); on rank 0 alone %.3f ms | stream: best() %.3f ms, best_words() %.3f ms; feed of all frames "
                         "%.3f ms, with the frame store %.3f ms"
                         % (r["B"], r["beams_ms"], r["words1_ms"], r["wordsB_ms"], r["mean_len"], r["pass_ms"], r["pass_frames_ms"],
                            r["pass_entropy_ms"], r["pass_entropy_frames_ms"], r["pass1_ms"], r["stream_best_ms"],
                            r["stream_best_words_ms"], r["stream_feed_ms"], r["stream_feed_conf_ms"]))
            continue
        if r["decoder"] in ("grid", "loop"):
            lines.append("%-7s B=%-4d G=%-3d %10.3f ms/call (min %.3f, max %.3f)  kernels %10.3f ms  %8.3f ms/point" %
                         (r["decoder"], r["B"], r["G"], r["ms_per_call"], r["min_ms"], r["max_ms"], r["kernel_ms"], r["ms_per_point"]))
            continue
        lines.append("%-11s B=%-4s %9.3f ms/batch (min %.3f, max %.3f)  %8.2f us/step" %
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
