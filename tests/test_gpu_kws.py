"""GPU checks of keyword spotting (csrc/ds2_kws.hip, keywords.KeywordSpotter) against the float32 numpy
restatement of the rule (tests/kws_reference.py).

Exact cases use scores that are multiples of 1/8 in [-12, 0] (test_gpu_ctc_align.py's device): every fp32 sum is exact, so hits,
their order, their scores, best and dropped must equal the restatement bit for bit, for log-probabilities and for logits (the
same grid plus a per-frame multiple of 1/8: the maximum cancels), contiguous and in the head's strided layout with NaN in every
frame past sizes[n].  Probabilities go through the device's logf, which is not numpy's: scores are held to
test_gpu_ctc_align.nll_bound and frames are compared on inputs where no decision can flip."""
import functools

import numpy as np
import pytest
import torch

import kws_reference as ref
from fixtures import DEV
from test_gpu_ctc_align import nll_bound
from test_kws_host import planted

pytestmark = pytest.mark.gpu
F32 = np.float32


def labels_for(C):
    return [chr(0x100 + i) for i in range(C)]           # class 0 is the blank


def words_of(ids, C):
    lab = labels_for(C)
    return [''.join(lab[i] for i in w) for w in ids]


def spotter(ids, C, thr, hold, max_hits=128):
    from deepspeech.pytorch_amd.keywords import KeywordSpotter
    thr = thr if isinstance(thr, list) else [thr] * len(ids)
    return KeywordSpotter(labels_for(C), list(zip(words_of(ids, C), thr)), hold=hold, blank_index=0, max_hits=max_hits), thr


def keyword(rng, L, C, repeats=True):
    """L labels that avoid the blank, with adjacent repeats now and then"""
    w = [int(rng.integers(1, C))]
    while len(w) < L:
        w.append(w[-1] if repeats and rng.random() < 0.25 else int(rng.integers(1, C)))
    return tuple(w)


def distinct(rng, lengths, C):
    seen, out = set(), []
    for L in lengths:
        w = keyword(rng, L, C)
        while w in seen:
            w = keyword(rng, L, C)
        seen.add(w)
        out.append(w)
    return out


def device_input(x, sizes, layout):
    """x (N, T, C) float32 with NaN in every frame past sizes[n]; "rows": the head's layout, a (T, N, Cpad) buffer seen as
    (N, T, C) -- the transposed view DeepSpeech.forward returns"""
    x = x.copy()
    for n, s in enumerate(sizes):
        x[n, s:] = np.nan
    N, T, C = x.shape
    if layout == "contig":
        return torch.from_numpy(x).to(DEV)
    buf = torch.full((T, N, C + 3), float("nan"), device=DEV)
    buf[:, :, :C] = torch.from_numpy(x).to(DEV).transpose(0, 1)
    v = buf[:, :, :C].transpose(0, 1)
    assert T == 0 or (not v.is_contiguous() and v.stride(2) == 1)
    return v


def as_tuples(dets):
    return [(d.index, d.start_frame, d.end_frame, d.score) for d in dets]


def want_tuples(hits):
    return [(k, b, e, float(s)) for k, b, e, s in ref.by_time(hits)]


def check_exact(x, sizes, ids, thr, hold, max_hits=128, kinds=("log_probs", "logits"), layouts=("contig", "rows"), seed=0):
    """spot() on every kind and layout against the restatement, bit for bit; returns the reference hits per clip"""
    N, T, C = x.shape
    sp, thr = spotter(ids, C, thr, hold, max_hits)
    want = [ref.spot(x[n, :sizes[n]], ids, thr, 0, hold, max_hits) for n in range(N)]
    shift = (np.random.default_rng(seed).integers(-80, 81, size=(N, T, 1)) / 8.0).astype(F32)
    for kind in kinds:
        for layout in layouts:
            xin = x + shift if kind == "logits" else x             # exact: multiples of 1/8 below 2^7
            got, best = sp.spot(device_input(xin, sizes, layout), torch.tensor(sizes), kind=kind, return_best=True)
            for n in range(N):
                hits, wbest, dropped = want[n]
                assert as_tuples(got[n]) == want_tuples(hits), (kind, layout, n)
                assert [(b.score, b.start_frame, b.end_frame) for b in best[n]] == [(float(s), b_, e) for s, b_, e in wbest], (kind, layout, n)
                assert sp.last_dropped[n] == dropped, (kind, layout, n)
    return want


def grid(seed, N, T, C):
    rng = np.random.default_rng(seed)
    return np.stack([ref.grid_log_probs(rng, T, C) for _ in range(N)]) if T else np.zeros((N, 0, C), F32)


# ---- exact: shapes ---------------------------------------------------------------------------------------------------------------
def test_lengths_1_2_63_64_three_clips_one_empty():
    rng = np.random.default_rng(1)
    ids = distinct(rng, [1, 2, 63, 64, 5, 3], 29)
    x = grid(1, 3, 150, 29)
    want = check_exact(x, [150, 0, 83], ids, -12.0, hold=3)
    assert want[1] == ([], [(ref.NINF, -1, -1)] * 6, 0)
    assert all(any(h[0] == k for h in want[0][0]) for k in range(6))       # every keyword, the 64-label one too, fires on noise


@pytest.mark.parametrize("lengths, C", [([64], 29), ([32, 32], 29), ([33, 32], 29), ([1] * 64, 300), ([1] * 65, 300), ([63, 1, 1], 29)])
def test_packings(lengths, C):
    rng = np.random.default_rng(len(lengths))
    ids = distinct(rng, lengths, C)
    x = grid(2, 1, 80, C)
    want = check_exact(x, [80], ids, -12.0, hold=2, kinds=("log_probs",), layouts=("rows",))
    assert len({h[0] for h in want[0][0]}) == len(lengths)


@pytest.mark.parametrize("K, C", [(1, 2), (200, 29), (7, 300)])
def test_keyword_counts_and_class_counts(K, C):
    rng = np.random.default_rng(K)
    ids = [(1, 1)] if C == 2 else distinct(rng, [2 + i % 5 for i in range(K)], C)
    x = grid(3, 1 if K == 200 else 3, 40, C)
    sizes = [40] if K == 200 else [40, 17, 1]
    check_exact(x, sizes, ids, -12.0, hold=4, layouts=("contig",) if K == 200 else ("contig", "rows"))


@pytest.mark.parametrize("T", [0, 1, 4, 5])
def test_clips_as_short_as_the_keyword(T):
    ids = [(1, 2, 3, 2, 1), (2,)]                         # L = 5: no path before frame L - 1
    x = grid(4, 2, T, 6)
    want = check_exact(x, [T, max(T - 1, 0)], ids, -12.0, hold=1)
    assert (want[0][1][0][0] > ref.NINF) == (T >= 5)


@pytest.mark.parametrize("hold", [1, 500])
def test_hold_of_one_frame_and_hold_beyond_the_clip(hold):
    ids = [(1,), (1, 2), (2, 2, 3)]
    x = grid(5, 2, 100, 5)
    want = check_exact(x, [100, 64], ids, -12.0, hold=hold, max_hits=128)
    n_hits = [len(w[0]) for w in want]
    assert n_hits == [3, 3] if hold == 500 else min(n_hits) > 40      # one merged hit per keyword, or one at almost every frame


def test_max_hits_of_one_counts_the_rest():
    ids = [(1,), (1, 2)]
    x = grid(6, 2, 60, 4)
    want = check_exact(x, [60, 60], ids, -12.0, hold=1, max_hits=1)
    assert all(len(w[0]) == 2 and w[2] > 20 for w in want)


def test_planted_occurrences_come_back_with_their_exact_spans():
    x = planted()[None]
    ids = [(3, 4, 3), (7, 7, 8)]                          # "CDC" as C C _ D C C at 50..55, "GGH" as G _ G H H at 120..124
    want = check_exact(x, [200], ids, -0.5, hold=25)
    assert want[0][0] == [(0, 50, 55, F32(0)), (1, 120, 124, F32(0))]


# ---- streaming ---------------------------------------------------------------------------------------------------------------------
STREAM_CHUNKS = [[1, 7, 64, 0, 65, 63], [64, 0, 65, 63, 1, 7], [0, 100, 0, 50, 50, 0]]


@functools.lru_cache(maxsize=None)
def _stream_case():
    rng = np.random.default_rng(8)
    x = np.stack([planted(seed=11), ref.grid_log_probs(rng, 200, 10), ref.grid_log_probs(rng, 200, 10)])
    ids = [(3, 4, 3), (7, 7, 8), (1,), (2, 2), (5, 6, 5, 6)]
    thr = [-0.5, -0.5, -12.0, -12.0, -12.0]
    return x, ids, thr


def _feed_all(ks, x, ids, thr, hold, kind="log_probs"):
    """feeds STREAM_CHUNKS to the device stream and to one RefStream per stream; checks every feed's hits; returns all hits"""
    refs = [ref.RefStream(ids, thr, 0, hold, ks.spotter.max_hits) for _ in range(3)]
    pos, got = [0, 0, 0], [[], [], []]
    for i in range(6):
        sizes = [STREAM_CHUNKS[n][i] for n in range(3)]
        Tc = max(sizes)
        block = np.full((3, Tc, x.shape[2]), np.nan, F32)
        for n in range(3):
            block[n, :sizes[n]] = x[n, pos[n]:pos[n] + sizes[n]]
        before = ks.h.state.clone()
        dets = ks.feed(torch.from_numpy(block).to(DEV), sizes, kind=kind, end=True if i == 5 else None)
        for n in range(3):
            want = refs[n].feed(x[n, pos[n]:pos[n] + sizes[n]], end=i == 5)
            assert as_tuples(dets[n]) == want_tuples(want), (i, n)               # in the feed in which rule 1 fires
            got[n] += as_tuples(dets[n])
            pos[n] += sizes[n]
            if sizes[n] == 0 and i < 5:                                          # a size of 0 leaves the stream's bits alone
                assert _same_bits(ks, before, ks.h.state, [n])
        assert ks.frames == pos
    assert [[(b.score, b.start_frame, b.end_frame) for b in row] for row in ks.best()] == \
        [[(float(s), b, e) for s, b, e in r.best] for r in refs]
    return got


def _same_bits(ks, a, b, streams):
    h = ks.h
    N, W, K = h.N, h.W, h.K
    parts = [(0, N * W * 256), (N * W * 256, N * K * 8), (N * W * 256 + N * K * 8, N * W)]
    return all(torch.equal(a[o:o + c].view(N, -1)[n], b[o:o + c].view(N, -1)[n]) for o, c in parts for n in streams)


@pytest.mark.parametrize("hold", [3, 25])
def test_chunked_feeds_give_the_one_shot_hits(hold):
    x, ids, thr = _stream_case()
    sp, _ = spotter(ids, 10, thr, hold)
    ks = sp.stream(3, DEV)
    got = _feed_all(ks, x, ids, thr, hold)
    one = sp.spot(torch.from_numpy(x).to(DEV), [200] * 3, kind="log_probs")
    for n in range(3):
        assert got[n] == as_tuples(one[n]), n
    assert (0, 50, 55, 0.0) in got[0] and (1, 120, 124, 0.0) in got[0]
    assert ks.dropped == [0, 0, 0]
    # reset of one stream leaves the others' bits alone, and the stream starts again as a fresh one
    before = ks.h.state.clone()
    ks.reset([1])
    assert _same_bits(ks, before, ks.h.state, [0, 2]) and ks.frames == [200, 0, 200]
    assert [b.score for b in ks.best()[1]] == [float("-inf")] * len(ids)
    again = ks.feed(torch.from_numpy(x).to(DEV), [0, 200, 0], kind="log_probs", end=[1])
    assert as_tuples(again[1]) == as_tuples(one[1]) and again[0] == [] and again[2] == []
    assert _same_bits(ks, before, ks.h.state, [0, 2])


def test_end_alone_and_feeds_of_no_frames():
    x, ids, thr = _stream_case()
    sp, _ = spotter(ids, 10, thr, 25)
    ks = sp.stream(3, DEV)
    assert ks.feed(torch.zeros((3, 0, 10), device=DEV)) == [[], [], []] and ks.end() == [[], [], []]
    ks.feed(torch.from_numpy(x[:, :60]).to(DEV), kind="log_probs")
    r = ref.RefStream(ids, thr, 0, 25, sp.max_hits)
    r.feed(x[0, :60])
    want = r.feed(x[0, :0], end=True)
    assert want and as_tuples(ks.end([0])[0]) == want_tuples(want)              # the planted hit at 50..55 is still held
    assert ks.end([0]) == [[], [], []] and ks.frames == [60, 60, 60]


# ---- probabilities -----------------------------------------------------------------------------------------------------------------
def test_probs_scores_within_the_bar_and_frames_where_no_decision_can_flip():
    rng = np.random.default_rng(12)
    N, T, C = 2, 160, 29
    # at least 3 labels each: thr_abs = -0.5 L is then more than 1 below the score 0 of an occurrence
    ids = [keyword(rng, 64, C), (3, 4, 3), (7, 7, 8), (9, 10, 9, 9), keyword(rng, 17, C)]
    thr = [-0.5] * len(ids)
    lp = rng.uniform(-48, -40, size=(N, T, C))
    win = rng.integers(0, C, size=(N, T))
    for n in range(N):                                     # plant every keyword once per clip, repeats through a blank frame
        t = 3 + n
        for w in ids:
            path = []
            for i, y in enumerate(w):
                path += ([0] if i and w[i - 1] == y else []) + [y] * int(rng.integers(1, 3))
            path = path[:T - t - 2]
            win[n, t:t + len(path)] = path
            t += len(path) + 2
            if t >= T - 4:
                break
    np.put_along_axis(lp, win[:, :, None], 0.0, axis=2)
    p = np.exp(lp).astype(F32)
    p[np.arange(N)[:, None], np.arange(T)[None], win] = F32(1) - (p.sum(2) - 1).astype(F32)       # a winner at probability near 1
    sizes = [T, T - 9]
    for n in range(N):
        for k, w in enumerate(ids):                        # on the reference: no end score within 1 of a threshold
            s = ref.end_scores(p[n, :sizes[n]], w, 0, "probs")
            thr_abs = ref.threshold_abs(thr[k], len(w))
            assert thr_abs >= -32 and not (np.abs(s - thr_abs) <= 1).any(), (n, k)
            assert ((s == 0) | (s < -40)).all()
    sp, _ = spotter(ids, C, thr, 5)
    total = 0
    for layout in ("contig", "rows"):
        got, best = sp.spot(device_input(p, sizes, layout), sizes, kind="probs", return_best=True)
        for n in range(N):
            hits, wbest, dropped = ref.spot(p[n, :sizes[n]], ids, thr, 0, 5, sp.max_hits, kind="probs")
            want = want_tuples(hits)
            assert [g[:3] for g in as_tuples(got[n])] == [h[:3] for h in want], (layout, n)
            for g, h in zip(as_tuples(got[n]), want):
                print("probs hit", g, h)
                assert abs(g[3] - h[3]) <= nll_bound(h[3])
            for b, (s, _, _) in zip(best[n], wbest):
                print("probs best", b.score, s)
                assert abs(b.score - float(s)) <= nll_bound(float(s)) if np.isfinite(s) else b.score == float(s)
            assert sp.last_dropped[n] == dropped == 0
            total += len(want)
    assert total >= 2 * 4


# ---- integration: the sessions feed the keyword stream what the decoder stream gets -------------------------------------------------
def _session_case():
    from deepspeech.pytorch_amd import synth
    from deepspeech.pytorch_amd.keywords import KeywordSpotter
    from fixtures import Fixture
    from test_gpu_model import build
    fx, lengths = Fixture("gru_uni_la"), [160, 155, 140]
    assert fx.cfg["hidden_size"] == 32 and fx.cfg["hidden_layers"] == 2 and not fx.cfg["bidirectional"]
    x = torch.from_numpy(synth.synth_batch(np.asarray(lengths), seed=11)[0]).to(DEV)
    m = build(fx, 32).eval()
    sp = KeywordSpotter.from_model(m, [("E", -8.0), ("TH", -6.0), (" A", -5.0), ("AA", -7.0)], hold=4, max_hits=64)
    assert sp.frame_seconds == 2 * m.spect_cfg.window_stride
    return fx, m, x, lengths, [54, 1, 2, 37, 66], sp


def _drive_pool(pool, x, lengths, chunks, order):
    """streams `order` join one tick after another on their own slots; returns per stream its concatenated output frames, the
    detections and the texts after every feed"""
    slot, fed = {}, {k: 0 for k in order}
    outs, dets, texts = {k: [] for k in order}, {k: [] for k in order}, {k: [] for k in order}
    tick = 0
    while any(fed[k] < lengths[k] for k in order):
        if tick < len(order):
            slot[order[tick]] = pool.open()
        rows = [k for k in slot if fed[k] < lengths[k]]
        lens = [min(chunks[tick % len(chunks)], lengths[k] - fed[k]) for k in rows]
        final = [k for k, c in zip(rows, lens) if fed[k] + c == lengths[k]]
        xc = torch.zeros((len(rows), 1, x.shape[2], max(lens)), device=DEV)
        for r, k in enumerate(rows):
            xc[r, :, :, :lens[r]] = x[k, :, :, fed[k]:fed[k] + lens[r]]
        text = pool.feed([slot[k] for k in rows], xc, lens, final=[slot[k] for k in final])
        for r, k in enumerate(rows):
            if pool.last_output.get(slot[k]) is not None:
                outs[k].append(pool.last_output[slot[k]])
            texts[k].append(text[r])
            fed[k] += lens[r]
            if pool.keywords is not None:
                dets[k] += pool.detections(slot[k])
        tick += 1
    for k in order:
        pool.close(slot[k])
    return outs, dets, texts, slot


def test_stream_pool_detections_equal_spot_on_the_slots_frames():
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.streaming import StreamPool
    fx, m, x, lengths, chunks, sp = _session_case()
    pool = StreamPool(m, D.GreedyDecoder(fx.labels), 3, keywords=sp)
    plain = StreamPool(m, D.GreedyDecoder(fx.labels), 3)
    s0 = plain.open()
    with pytest.raises(ValueError, match="keywords="):
        plain.detections(s0)
    plain.close(s0)
    total = 0
    for order in ([0, 1, 2], [2, 0]):                      # the second round re-uses the slots after close / open
        outs, dets, texts, _ = _drive_pool(pool, x, lengths, chunks, order)
        _, _, plain_texts, _ = _drive_pool(plain, x, lengths, chunks, order)
        assert texts == plain_texts                        # the transcripts do not know about the keyword stream
        for k in order:
            frames = torch.cat(outs[k])[None]
            want = sp.spot(frames, [frames.shape[1]])[0]
            assert dets[k] == want, (order, k)
            assert sp.last_dropped == [0]
            total += len(want)
    assert total > 0


def test_streaming_transcriber_detections_equal_spot_on_its_frames():
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.streaming import StreamingTranscriber
    fx, m, x, lengths, chunks, sp = _session_case()
    x, lengths = x[:2], lengths[:2]
    st = StreamingTranscriber(m, D.GreedyDecoder(fx.labels), carry_context=True, keywords=sp)
    for _ in range(2):                                     # the second utterance after reset()
        pos, outs, dets = 0, [[], []], [[], []]
        for i, c in enumerate(chunks):
            last = i == len(chunks) - 1
            st.feed(x[:, :, :, pos:pos + c].contiguous(), [g - pos for g in lengths] if last else [c] * 2, final=last)
            if st.last_output is not None:
                probs, sizes = st.last_output
                for n in range(2):
                    outs[n].append(probs[n, :int(sizes[n])])
            for n, d in enumerate(st.detections()):
                dets[n] += d
            pos += c
        for n in range(2):
            frames = torch.cat(outs[n])[None]
            want = sp.spot(frames, [frames.shape[1]])[0]
            assert dets[n] == want and len(want) > 0, n
            assert want[0].start_s == want[0].start_frame * sp.frame_seconds
        st.reset()
