"""GPU checks of the device beam search with hot words (ds2_beam_decode_hot, ds2_beam_decode_lm_hot, ops.beam_decode_hot /
beam_decode_lm_hot, decoder.BeamCTCDecoder with hotwords) against the numpy restatement of the rules
(tests/beam_hot_reference.py, itself pinned by tests/test_beam_hot_reference.py).  The rule of comparison is that of
tests/test_gpu_beam_lm.py: the kernel and the fp32 restatement evaluate the same operations, so label sequences, lengths and
offsets of all beams must be identical; scores are held to 1e-4 relative (equal bits expected) and rank order is compared
wherever adjacent totals are more than 1e-6 apart.  The grid and its inputs are tests/beam_hot_cases.py; the host file asserts on
the same inputs that every rule fires and that the top beam is compared by rank in at least 90 % of the utterances."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import beam_hot_cases as HC
from beam_hot_reference import beam_search_hot

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _lm_tables(name):
    from deepspeech.pytorch_amd import lm
    labels = HC.labels()
    wt, gt = lm.build_tables(HC.lm(name), labels, 0, labels.index(' '))
    return torch.from_numpy(wt).to(DEV), torch.from_numpy(gt).to(DEV)


def _hot(phrases, weight=None):
    """the device table of phrases (weight: every phrase gets this one)"""
    from deepspeech.pytorch_amd import hotwords
    if weight is not None:
        phrases = [(p if isinstance(p, str) else p[0], weight) for p in phrases]
    return torch.from_numpy(hotwords.build_table(phrases, HC.labels(), 0, HC.DEFAULT_WEIGHT)).to(DEV)


def _decode(view, sizes, B, name, lexicon, top_n, cutoff_prob, alpha, beta, ht):
    from deepspeech.pytorch_amd import ops
    sp = HC.labels().index(' ')
    sz = None if sizes is None else torch.from_numpy(sizes)
    if name is None:
        return ops.beam_decode_hot(view, sz, 0, B, top_n, cutoff_prob, sp, ht)
    wt, gt = _lm_tables(name)
    m = HC.lm(name)
    return ops.beam_decode_lm_hot(view, sz, 0, B, top_n, cutoff_prob, sp, wt, gt, m.order, m.bos, alpha, beta, lexicon, ht,
                                  HC.HOT_OOV_LOGP)


def _check(toks, offs, scores, acoustic, refs, B):
    for n, ref in enumerate(refs):
        rb = ref["beams"]
        alive = int(torch.isfinite(scores[n]).sum())
        assert alive == len(rb), (n, alive, len(rb))
        got = [(tuple(toks[n][b]), tuple(offs[n][b].tolist()), float(scores[n, b]), float(acoustic[n, b])) for b in range(alive)]
        for b in range(alive, B):
            assert toks[n][b] == [] and scores[n, b] == float("inf") and acoustic[n, b] == float("inf")
        assert len({g[0] for g in got}) == alive
        gd, rd = {g[0]: g for g in got}, {r[0]: r for r in rb}
        assert set(gd) == set(rd), n
        for lab, (_, fr, s, a) in rd.items():
            assert gd[lab][1] == fr, (n, lab, gd[lab][1], fr)
            assert abs(gd[lab][2] - s) <= 1e-4 * max(1.0, abs(s)), (n, lab, gd[lab][2], s)
            assert abs(gd[lab][3] - a) <= 1e-4 * max(1.0, abs(a)), (n, lab, gd[lab][3], a)
        for b in range(alive):
            if not HC.near(rb, b):
                assert got[b][0] == rb[b][0], (n, b)


@pytest.mark.parametrize("case", HC.GRID, ids=lambda c: "-".join(str(v) for v in c))
def test_kernel_matches_restatement(case):
    N, T, B, name, lexicon, top_n, cutoff_prob, strided, alpha, beta = case
    p, sizes, refs = HC.case(*case)
    if strided:
        view = torch.from_numpy(np.ascontiguousarray(p.transpose(1, 0, 2))).to(DEV).transpose(0, 1)
        assert not view.is_contiguous()
    else:
        view = torch.from_numpy(p).to(DEV)
    toks, offs, scores, acoustic = _decode(view, sizes, B, name, lexicon, top_n, cutoff_prob, alpha, beta, _hot(HC.PHRASES[name]))
    assert scores.shape == (N, B) and acoustic.shape == (N, B) and len(toks) == N and all(len(t) == B for t in toks)
    _check(toks, offs, scores, acoustic, refs, B)


def _same_bits(a, b):
    return a[0] == b[0] and all(torch.equal(x, y) for u, v in zip(a[1], b[1]) for x, y in zip(u, v)) and \
        torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


@pytest.mark.parametrize("N,T,B,top_n,cutoff_prob", [(3, 17, 16, 40, 1.0), (3, 60, 256, 40, 0.9), (2, 60, 2, 5, 1.0)])
def test_zero_weights_give_the_bits_of_the_entries_without_hot_words(N, T, B, top_n, cutoff_prob):
    from deepspeech.pytorch_amd import ops
    p, sizes = HC.inputs(5 + N + T, N, T, "toy3")
    view, sz = torch.from_numpy(p).to(DEV), torch.from_numpy(sizes)
    sp = HC.labels().index(' ')
    # without an LM any phrase will do; with one every phrase word is in the vocabulary, so that no word event is covered
    plain = ops.beam_decode(view, sz, 0, B, top_n, cutoff_prob)
    hot = ops.beam_decode_hot(view, sz, 0, B, top_n, cutoff_prob, sp, _hot(HC.PHRASES["toy3"], 0.0))
    assert _same_bits(plain, hot) and torch.equal(hot[2].view(torch.int32), hot[3].view(torch.int32))
    wt, gt = _lm_tables("toy3")
    m = HC.lm("toy3")
    ht = _hot(["THE CAT", "THE CAN", "TENT", "RED HAT", "A"], 0.0)
    for lexicon in (False, True):
        lm = ops.beam_decode_lm(view, sz, 0, B, top_n, cutoff_prob, sp, wt, gt, m.order, m.bos, 1.1, 0.4, lexicon)
        both = ops.beam_decode_lm_hot(view, sz, 0, B, top_n, cutoff_prob, sp, wt, gt, m.order, m.bos, 1.1, 0.4, lexicon, ht, -11.5)
        assert _same_bits(lm, both) and torch.equal(lm[3].view(torch.int32), both[3].view(torch.int32))


def _clip(text):
    """every label of text as a 0.98 row, a blank row after each"""
    labels = HC.labels()
    frames = []
    for ch in text:
        frames += [labels.index(ch), 0]
    p = np.full((len(frames), len(labels)), 0.02 / (len(labels) - 1), np.float32)
    p[np.arange(len(frames)), frames] = 0.98
    return (p / p.sum(-1, keepdims=True)).astype(np.float32)[None]


def test_decoder_hotwords_empty_list_set_hotwords_and_the_grid():
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    labels = HC.labels()
    p, sizes = HC.inputs(11, 2, 60, "toy3")
    probs, sz = torch.from_numpy(p).to(DEV), torch.from_numpy(sizes)
    plain = BeamCTCDecoder(labels, beam_width=16).decode_beams(probs, sz)
    calls = []
    real = ops.beam_decode_hot
    dec = BeamCTCDecoder(labels, beam_width=16, hotwords=[])
    try:
        ops.beam_decode_hot = lambda *a, **k: calls.append(1) or real(*a, **k)
        empty = dec.decode_beams(probs, sz)                                   # hotwords=[] takes the old path
        assert not calls and empty[0] == plain[0] and torch.equal(empty[2], plain[2])
        dec.set_hotwords(["NEW YORK", ("TENT", 3.0)])                         # changes the next call
        hot = dec.decode_beams_detailed(probs, sz)
        assert len(calls) == 1
    finally:
        ops.beam_decode_hot = real
    table = HC.hot_table(["NEW YORK", ("TENT", 3.0)])
    for n in range(2):
        ref = beam_search_hot(p[n], sizes[n], 0, 16, 40, 1.0, table)["beams"]
        assert hot[0][n][0] == ''.join(labels[c] for c in ref[0][0])
        assert abs(float(hot[2][n, 0]) - ref[0][2]) <= 1e-4 * max(1.0, abs(ref[0][2]))
        assert abs(float(hot[3][n, 0]) - ref[0][3]) <= 1e-4 * max(1.0, abs(ref[0][3]))
    assert not torch.equal(hot[2], plain[2])                                  # the boost is in the scores
    strings, offsets = dec.decode(torch.from_numpy(p).double(), None)         # a host tensor and no sizes
    assert len(strings) == 2 and all(len(s) == 16 for s in strings) and offsets[0][0].dtype == torch.int32
    dec.set_hotwords(None)
    back = dec.decode_beams(probs, sz)
    assert back[0] == plain[0] and torch.equal(back[2], plain[2])
    # the weight search refuses hot words
    lmdec = BeamCTCDecoder(labels, os.path.join(HC.GOLDEN, "toy3.arpa"), 1.0, 1.0, beam_width=8, hotwords=["NEW YORK"])
    with pytest.raises(ValueError, match="hot words"):
        lmdec.decode_grid(probs, sz, [(1.0, 1.0), (0.5, 2.0)])
    lmdec.set_hotwords([])
    assert len(lmdec.decode_grid(probs, sz, [(1.0, 1.0), (0.5, 2.0)])[0]) == 2


def test_out_of_vocabulary_hot_phrase_wins_in_lexicon_mode():
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    labels = HC.labels()
    text = "HE SAW NEW YORK"
    p = _clip(text)
    assert "NEW" not in HC.lm("toy3").word_id and "YORK" not in HC.lm("toy3").word_id
    probs = torch.from_numpy(p).to(DEV)
    path = os.path.join(HC.GOLDEN, "toy3.arpa")
    dec = BeamCTCDecoder(labels, path, 1.0, 1.0, beam_width=16, lexicon=True)
    without = dec.decode_beams(probs)[0][0][0]
    assert "NEW" not in without.split(' ') and "YORK" not in without                 # the lexicon cannot spell it
    dec.set_hotwords(["NEW YORK"])
    strings, offsets, scores, acoustic = dec.decode_beams_detailed(probs)
    assert strings[0][0] == text and len(offsets[0][0]) == len(text)
    # the restatement says the same, to the bit pattern of the rules: 2 word events at hot_oov_logp, 7 labels at 2.0
    ref = beam_search_hot(p[0], p.shape[1], 0, 16, 40, 1.0, HC.hot_table(["NEW YORK"]), HC.scorer("toy3", 1.0, 1.0, True))["beams"]
    assert ''.join(labels[c] for c in ref[0][0]) == text and abs(float(scores[0, 0]) - ref[0][2]) <= 1e-4 * abs(ref[0][2])
    # a near miss earns nothing: on NEW YORKER the plain search and the boosted one agree on the top beam without an LM, and the
    # boosted total of that beam is its acoustic score (the beams kept on the way differ, so the masses need not be equal bits)
    q = torch.from_numpy(_clip("NEW YORKER SAT")).to(DEV)
    a = BeamCTCDecoder(labels, beam_width=8).decode_beams(q)
    b = BeamCTCDecoder(labels, beam_width=8, hotwords=[("NEW YORK", 0.5)]).decode_beams_detailed(q)   # 3.5 buys no wrong frame (7.2)
    assert a[0][0][0] == b[0][0][0] == "NEW YORKER SAT" and float(b[2][0, 0]) == float(b[3][0, 0])
    assert abs(float(a[2][0, 0]) - float(b[2][0, 0])) < 0.05


def test_argument_errors():
    from deepspeech.pytorch_amd import _lib, ops
    labels = HC.labels()
    ht = _hot(["NEW YORK"])
    p = torch.from_numpy(HC.inputs(1, 2, 10, "toy3")[0]).to(DEV)
    sp = labels.index(' ')
    good = dict(probs=p, sizes=None, blank=0, beam_width=4, cutoff_top_n=40, cutoff_prob=1.0, space=sp, hot_table=ht)
    ops.beam_decode_hot(**good)
    for bad in (dict(space=0), dict(space=len(labels)), dict(beam_width=257), dict(hot_table=ht[:3]), dict(hot_table=ht.cpu()),
                dict(hot_table=ht.to(torch.int32)), dict(hot_table=None)):
        with pytest.raises(ValueError):
            ops.beam_decode_hot(**dict(good, **bad))
    wt, gt = _lm_tables("toy3")
    m = HC.lm("toy3")
    with pytest.raises(ValueError, match="hot_oov_logp"):
        ops.beam_decode_lm_hot(p, None, 0, 4, 40, 1.0, sp, wt, gt, m.order, m.bos, 1.0, 1.0, True, ht, float("nan"))
    with pytest.raises(ValueError, match="hot_table"):
        ops.beam_stream_open(2, 10, len(labels), 0, 4, 40, 1.0, DEV, None, dict(space=sp, table=ht.cpu()))
    # the raw ABI
    lib = _lib.load()
    N, T, C, B = 2, 10, len(labels), 4
    buf = torch.empty((2, N, B, T), dtype=torch.int32, device=DEV)
    lens = torch.empty((N, B), dtype=torch.int32, device=DEV)
    scores = torch.empty((N, B), dtype=torch.float32, device=DEV)
    ws = torch.empty(lib.ds2_beam_ws_bytes(N, T, B), dtype=torch.uint8, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(space=sp, htab=ht.data_ptr(), hslots=ht.shape[0], blank=0):
        return lib.ds2_beam_decode_hot(p.data_ptr(), p.stride(0), p.stride(1), N, T, C, None, blank, B, 40, 1.0, space, htab, hslots,
                                       buf[0].data_ptr(), buf[1].data_ptr(), lens.data_ptr(), scores.data_ptr(), None, ws.data_ptr(), st)

    def raw_lm(hslots=ht.shape[0], oov=-11.5, order=m.order):
        return lib.ds2_beam_decode_lm_hot(p.data_ptr(), p.stride(0), p.stride(1), N, T, C, None, 0, B, 40, 1.0, sp, wt.data_ptr(),
                                          wt.shape[0], gt.data_ptr(), gt.shape[0], order, m.bos, 1.0, 1.0, 1, ht.data_ptr(), hslots, oov,
                                          buf[0].data_ptr(), buf[1].data_ptr(), lens.data_ptr(), scores.data_ptr(), None, ws.data_ptr(), st)

    assert raw() == 0 and raw_lm() == 0
    torch.cuda.synchronize()
    for kw in (dict(space=-1), dict(space=C), dict(space=3, blank=3), dict(htab=None), dict(hslots=ht.shape[0] - 1), dict(hslots=0)):
        assert raw(**kw) == 1002, kw                                          # DS2_ERR_ARG
    for kw in (dict(hslots=3), dict(oov=float("inf")), dict(oov=float("nan")), dict(order=6)):
        assert raw_lm(**kw) == 1002, kw
    # the flag word of the stream's size queries: 0 and 1 as before, bit 1 adds the hot-word fields
    assert lib.ds2_beam_stream_state_stride(4, 0) == 256 and lib.ds2_beam_stream_state_stride(4, 1) == 512
    assert lib.ds2_beam_stream_state_stride(256, 2) == 16 + 64 * 256 + 240 and lib.ds2_beam_stream_state_stride(4, 4) == 0
    assert lib.ds2_beam_stream_state_stride(1, 3) == 256 and lib.ds2_beam_stream_state_stride(256, 3) == 23808
    assert lib.ds2_beam_stream_bytes(2, 16, 10, 3) > lib.ds2_beam_stream_bytes(2, 16, 10, 1) > 0 == lib.ds2_beam_stream_bytes(2, 16, 10, 8)
