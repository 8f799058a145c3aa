"""GPU checks of the device beam search with a word n-gram language model (ds2_beam_decode_lm, ops.beam_decode_lm,
decoder.BeamCTCDecoder with lm_path) against the numpy restatement of its rules (tests/beam_lm_reference.py, itself pinned by
tests/test_beam_lm_reference.py).  As in tests/test_gpu_beam.py the kernel and the fp32 restatement evaluate the same operations,
so label sequences, lengths and offsets of all beams must be identical; scores are held to 1e-4 relative (equal bits expected) and
rank order is compared wherever adjacent totals are more than 1e-6 apart.  test_top_beam_is_compared_by_rank makes sure that this
last rule does not hide the top beam: it must have been compared by rank in at least 90 % of the grid's utterances.

The inputs contain words: every utterance is a sentence over the fixture's vocabulary planted as peaky rows (with noise, so that
misspellings compete), followed by random peaky rows."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from beam_lm_reference import Scorer, beam_search_lm
from beam_reference import beam_search
from fixtures import Fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm")
SENTENCES = {
    "toy3": ["THE CAT SAT ON THE MAT", "IT'S A BIG RED HAT", "AN ANT AND A CAT SAT", "HE SAW THE DOG", "A CAT AND A DOG RAN",
             "THEY SAT IN THE TENT", "AT TEN SHE ATE A NUT", "THE HAT IS RED"],
    "toy5": ["A AN A NA", "AN A NAN A ANNA", "NA NA NAN", "ANNA AN A", "A NA AN ANNA"],
}
SENTENCES["toy1"] = SENTENCES["toy3"]


def _labels():
    from deepspeech.pytorch_amd.configs import LABELS
    return LABELS


@functools.lru_cache(maxsize=None)
def _lm(name):
    from deepspeech.pytorch_amd import lm
    return lm.load_arpa(os.path.join(GOLDEN, name + ".arpa"))


@functools.lru_cache(maxsize=None)
def _tables(name):
    from deepspeech.pytorch_amd import lm
    labels = _labels()
    wt, gt = lm.build_tables(_lm(name), labels, 0, labels.index(' '))
    return torch.from_numpy(wt).to(DEV), torch.from_numpy(gt).to(DEV)


def _softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def _planted(rng, T, sents, labels, peak=5.0, noise=1.5):
    """(T, C) probabilities: sentences drawn from sents, their labels one or two frames each (a blank between equal neighbours and
    after some labels) as peaky rows with noise over the first nine tenths of the frames, then random peaky rows"""
    path, prev = [], -1
    while len(path) < 0.9 * T:
        for ch in sents[int(rng.integers(0, len(sents)))] + " ":
            c = labels.index(ch)
            if c == prev or rng.random() < 0.3:
                path.append(0)
            path += [c] * int(rng.integers(1, 3))
            prev = c
    z = rng.standard_normal((T, len(labels))) * 3.0
    n = min(T, len(path), max(int(0.9 * T), 2))
    z[:n] = rng.standard_normal((n, len(labels))) * noise
    z[np.arange(n), path[:n]] += peak
    return _softmax(z)


def _inputs(seed, N, T, name):
    rng = np.random.default_rng(seed)
    labels = _labels()
    p = np.stack([_planted(rng, T, SENTENCES[name] if T > 2 else ["A"], labels) for _ in range(N)])
    sizes = rng.integers(1, T + 1, size=N)
    sizes[0] = T
    if N >= 3:
        sizes[1] = 0
    return p, sizes.astype(np.int32)


# (N, T, B, model, lexicon, cutoff_prob, strided (T, N, C) view, alpha, beta)
GRID = [
    (1, 2, 256, "toy3", False, 1.0, False, 1.2, 0.8),
    (1, 17, 256, "toy3", False, 1.0, False, 1.0, 1.0),
    (1, 200, 128, "toy5", True, 1.0, False, 0.8, 1.5),
    (1, 200, 128, "toy5", True, 0.9, False, 0.8, 1.5),     # the lexicon and the cut leave a frame without a candidate: no beam survives
    (3, 2, 10, "toy1", False, 1.0, True, 1.5, 0.5),
    (3, 2, 1, "toy3", True, 1.0, False, 1.0, 1.0),
    (3, 17, 10, "toy3", True, 1.0, True, 1.3, 0.7),
    (3, 17, 128, "toy5", False, 0.9, False, 0.5, 2.0),
    (3, 200, 256, "toy1", True, 1.0, False, 1.0, 1.0),
    (3, 200, 10, "toy3", False, 0.9, True, 0.9, 1.1),
    (8, 17, 1, "toy1", False, 1.0, False, 2.0, 0.0),
    (8, 17, 256, "toy3", True, 0.9, False, 1.1, 0.3),
    (8, 200, 10, "toy5", False, 1.0, False, 1.4, 0.6),
    (8, 200, 128, "toy3", False, 1.0, True, 0.7, 1.9),
    (8, 2, 128, "toy5", True, 1.0, False, 1.0, 1.0),
]


@functools.lru_cache(maxsize=None)
def _case(N, T, B, name, lexicon, cutoff_prob, strided, alpha, beta):
    """the case's inputs and the restatement's result per utterance (made once, on the CPU)"""
    p, sizes = _inputs(N * 1000 + T * 7 + B, N, T, name)
    sc = Scorer(_lm(name), _labels(), 0, alpha, beta, lexicon, np.float32)
    refs = [beam_search_lm(p[n], sizes[n], 0, B, 40, cutoff_prob, sc) for n in range(N)]
    return p, sizes, refs


def _near(rb, b):
    return (b > 0 and rb[b][2] - rb[b - 1][2] <= 1e-6 * max(1.0, abs(rb[b][2]))) or \
        (b + 1 < len(rb) and rb[b + 1][2] - rb[b][2] <= 1e-6 * max(1.0, abs(rb[b][2])))


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
            if not _near(rb, b):
                assert got[b][0] == rb[b][0], (n, b)


@pytest.mark.parametrize("case", GRID, ids=lambda c: "-".join(str(v) for v in c))
def test_kernel_matches_restatement(case):
    from deepspeech.pytorch_amd import ops
    N, T, B, name, lexicon, cutoff_prob, strided, alpha, beta = case
    p, sizes, refs = _case(*case)
    assert sum(r["word_events"] for r in refs) >= 1
    if not lexicon:
        assert sum(r["oov_events"] for r in refs) >= 1
    if strided:
        view = torch.from_numpy(np.ascontiguousarray(p.transpose(1, 0, 2))).to(DEV).transpose(0, 1)
        assert not view.is_contiguous()
    else:
        view = torch.from_numpy(p).to(DEV)
    wt, gt = _tables(name)
    m = _lm(name)
    labels = _labels()
    toks, offs, scores, acoustic = ops.beam_decode_lm(view, torch.from_numpy(sizes), 0, B, 40, cutoff_prob, labels.index(' '), wt, gt,
                                                      m.order, m.bos, alpha, beta, lexicon)
    assert scores.shape == (N, B) and acoustic.shape == (N, B) and len(toks) == N and all(len(t) == B for t in toks)
    _check(toks, offs, scores, acoustic, refs, B)


def test_top_beam_is_compared_by_rank():
    """the 1e-6 rule of the rank comparison must not hide the top beam: it is compared in at least 90 % of the grid's utterances"""
    compared = total = 0
    for case in GRID:
        for ref in _case(*case)[2]:
            total += 1
            compared += len(ref["beams"]) > 0 and not _near(ref["beams"], 0)
    assert total == sum(c[0] for c in GRID) and compared >= 0.9 * total, (compared, total)


@pytest.mark.parametrize("N,T,B,top_n,cutoff_prob", [(3, 17, 10, 40, 1.0), (8, 200, 128, 40, 0.9), (3, 200, 256, 5, 1.0)])
def test_zero_weights_in_open_mode_equal_the_entry_without_lm(N, T, B, top_n, cutoff_prob):
    from deepspeech.pytorch_amd import ops
    p, sizes = _inputs(5 + N + T, N, T, "toy3")
    view, sz = torch.from_numpy(p).to(DEV), torch.from_numpy(sizes)
    wt, gt = _tables("toy3")
    m = _lm("toy3")
    a = ops.beam_decode(view, sz, 0, B, top_n, cutoff_prob)
    b = ops.beam_decode_lm(view, sz, 0, B, top_n, cutoff_prob, _labels().index(' '), wt, gt, m.order, m.bos, 0.0, 0.0, False)
    assert a[0] == b[0]
    assert all(torch.equal(x, y) for u, v in zip(a[1], b[1]) for x, y in zip(u, v))
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)) and torch.equal(b[2].view(torch.int32), b[3].view(torch.int32))


def _flip_input():
    """THE CAT SAT with K a little likelier than C at the C: without an LM the best string is the misspelling"""
    labels = _labels()
    path = [labels.index(ch) for ch in "THE CAT SAT"]
    frames = []
    for c in path:
        frames += [c, 0]
    p = np.full((len(frames), len(labels)), 0.02 / (len(labels) - 1), np.float32)
    p[np.arange(len(frames)), frames] = 0.98
    for t, c in enumerate(frames):
        if c == labels.index("C"):
            p[t, c], p[t, labels.index("K")] = 0.40, 0.58
    return (p / p.sum(-1, keepdims=True)).astype(np.float32)[None]


def test_language_model_flips_a_planted_misspelling():
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    labels = _labels()
    p = _flip_input()
    T = p.shape[1]
    text = lambda lab: ''.join(labels[c] for c in lab)
    # on the CPU first
    plain = beam_search(p[0], T, 0, 16, 40, 1.0)["beams"]
    assert text(plain[0][0]) == "THE KAT SAT" and "KAT" not in _lm("toy3").word_id
    for lexicon in (False, True):
        ref = beam_search_lm(p[0], T, 0, 16, 40, 1.0, Scorer(_lm("toy3"), labels, 0, 1.0, 1.0, lexicon))["beams"]
        assert text(ref[0][0]) == "THE CAT SAT"
    # then on the device
    probs = torch.from_numpy(p).to(DEV)
    assert BeamCTCDecoder(labels, beam_width=16).decode(probs)[0][0][0] == "THE KAT SAT"
    for lexicon in (False, True):
        dec = BeamCTCDecoder(labels, os.path.join(GOLDEN, "toy3.arpa"), 1.0, 1.0, beam_width=16, lexicon=lexicon)
        strings, offsets, scores, acoustic = dec.decode_beams_detailed(probs)
        assert strings[0][0] == "THE CAT SAT" and len(offsets[0][0]) == 11
        assert float(acoustic[0, 0]) > float(plain[0][2])                    # acoustically worse than the misspelling


@pytest.mark.parametrize("name,B", [("toy3", 64), ("toy5", 256), ("toy1", 10)])
def test_lexicon_mode_outputs_only_vocabulary_words(name, B):
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    p, sizes = _inputs(77, 6, 120, name)
    dec = BeamCTCDecoder(_labels(), os.path.join(GOLDEN, name + ".arpa"), 1.0, 1.0, beam_width=B)
    strings, _, scores = dec.decode_beams(torch.from_numpy(p).to(DEV), torch.from_numpy(sizes))
    vocab, seen = set(_lm(name).words), 0
    for n in range(len(strings)):
        for b in range(int(torch.isfinite(scores[n]).sum())):
            words = strings[n][b].split(' ')
            assert all(w in vocab for w in words[:-1]), (n, b, strings[n][b])
            assert any(v.startswith(words[-1]) for v in vocab)
            seen += len(words) - 1
    assert seen > 100


def test_decoder_with_language_model_shapes_host_input_and_repeatability():
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    labels = _labels()
    p, _ = _inputs(3, 2, 60, "toy3")
    dec = BeamCTCDecoder(labels, lm_path=os.path.join(GOLDEN, "toy3.arpa"), alpha=1.2, beta=0.9, beam_width=8)
    strings, offsets = dec.decode(torch.from_numpy(p).double())             # a host tensor and no sizes, as run_transcribe passes
    assert len(strings) == 2 and all(len(s) == 8 for s in strings) and all(len(o) == 8 for o in offsets)
    sc = Scorer(_lm("toy3"), labels, 0, 1.2, 0.9, True)
    for n in range(2):
        ref = beam_search_lm(p[n], 60, 0, 8, 40, 1.0, sc)["beams"]
        assert strings[n][0] == ''.join(labels[c] for c in ref[0][0])
        assert offsets[n][0].dtype == torch.int32 and tuple(offsets[n][0].tolist()) == ref[0][1]
    again = dec.decode_beams(torch.from_numpy(p).to(DEV), torch.tensor([60, 60]))
    assert again[0] == strings and again[2].shape == (2, 8) and bool((again[2][:, 1:] >= again[2][:, :-1]).all())
    third = dec.decode_beams(torch.from_numpy(p).to(DEV), torch.tensor([60, 60]))
    assert third[0] == again[0] and torch.equal(third[2], again[2])
    assert all(torch.equal(x, y) for u, v in zip(third[1], again[1]) for x, y in zip(u, v))
    assert len(dec._tables) == 1                                             # built once, kept


def test_validation_step_with_language_model_decoder():
    from test_gpu_beam import _model
    from deepspeech.pytorch_amd import decoder as D
    fx = Fixture("gru_bi_mid")
    m = _model(fx).eval()
    beam = D.BeamCTCDecoder(fx.labels, os.path.join(GOLDEN, "toy3.arpa"), 0.5, 1.0, beam_width=10, lexicon=False)
    tgt = D.GreedyDecoder(fx.labels)
    m.attach_evaluation(beam, D.WordErrorRate(decoder=beam, target_decoder=tgt), D.CharErrorRate(decoder=beam, target_decoder=tgt))
    logged = {}
    m.log = lambda k, v, **kw: logged.__setitem__(k, v)
    inputs, targets, pct, tsz = fx.batch()
    with torch.no_grad():
        m.validation_step((torch.from_numpy(inputs), torch.from_numpy(targets), torch.from_numpy(pct.copy()), torch.from_numpy(tsz)), 0)
    assert set(logged) == {"wer", "cer"} and all(np.isfinite(float(v)) and float(v) >= 0 for v in logged.values())


def test_argument_errors():
    from deepspeech.pytorch_amd import _lib, ops
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    labels = _labels()
    path = os.path.join(GOLDEN, "toy3.arpa")
    with pytest.raises(ValueError, match="space label"):
        BeamCTCDecoder([c for c in labels if c != ' '], lm_path=path)
    with pytest.raises(ValueError, match="ARPA"):
        BeamCTCDecoder(labels, lm_path=os.path.join(GOLDEN, "..", "single_sample.npz"))
    wt, gt = _tables("toy3")
    m = _lm("toy3")
    p = torch.from_numpy(_inputs(1, 2, 10, "toy3")[0]).to(DEV)
    sp = labels.index(' ')
    good = dict(probs=p, sizes=None, blank=0, beam_width=4, cutoff_top_n=40, cutoff_prob=1.0, space=sp, word_table=wt, ngram_table=gt,
                order=m.order, bos=m.bos, alpha=1.0, beta=1.0)
    ops.beam_decode_lm(**good)
    for bad in (dict(order=6), dict(order=0), dict(space=0), dict(space=len(labels)), dict(beam_width=257), dict(word_table=wt[:3]),
                dict(ngram_table=gt.cpu()), dict(word_table=wt.to(torch.int32)), dict(bos=-1)):
        with pytest.raises(ValueError):
            ops.beam_decode_lm(**dict(good, **bad))
    # the raw ABI
    lib = _lib.load()
    N, T, C, B = 2, 10, len(labels), 4
    buf = torch.empty((2, N, B, T), dtype=torch.int32, device=DEV)
    lens = torch.empty((N, B), dtype=torch.int32, device=DEV)
    scores = torch.empty((N, B), dtype=torch.float32, device=DEV)
    ws = torch.empty(lib.ds2_beam_ws_bytes(N, T, B), dtype=torch.uint8, device=DEV)

    def raw(space=sp, wtab=wt.data_ptr(), wslots=wt.shape[0], gtab=gt.data_ptr(), gslots=gt.shape[0], order=m.order, blank=0):
        return lib.ds2_beam_decode_lm(p.data_ptr(), p.stride(0), p.stride(1), N, T, C, None, blank, B, 40, 1.0, space, wtab, wslots,
                                      gtab, gslots, order, m.bos, 1.0, 1.0, 1, buf[0].data_ptr(), buf[1].data_ptr(), lens.data_ptr(),
                                      scores.data_ptr(), None, ws.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    assert raw() == 0
    torch.cuda.synchronize()
    for kw in (dict(order=6), dict(order=0), dict(space=-1), dict(space=C), dict(space=3, blank=3), dict(wtab=None), dict(gtab=None),
               dict(wslots=wt.shape[0] - 1), dict(gslots=0)):
        assert raw(**kw) == 1002, kw                                          # DS2_ERR_ARG
