"""GPU check of lm_search.LMGridSearch and BeamCTCDecoder.decode_grid against a loop over the points that builds one
BeamCTCDecoder(alpha, beta) per point and feeds the two host metric classes: the same integers go through the same division, so
the rates are equal as floats."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_beam_lm import DEV, GOLDEN, SENTENCES, _inputs, _labels

pytestmark = pytest.mark.gpu
POINTS = [(0.0, 0.0), (0.5, 0.5), (1.0, 1.0), (1.5, 0.2), (2.0, 2.0), (1.0, 1.0)]
ARPA = os.path.join(GOLDEN, "toy3.arpa")
KW = dict(beam_width=10, lexicon=False)


def _batch(seed, N, T):
    rng = np.random.default_rng(seed)
    labels = _labels()
    p, sizes = _inputs(seed, N, T, "toy3")
    sents = [SENTENCES["toy3"][int(rng.integers(0, len(SENTENCES["toy3"])))] for _ in range(N)]
    targets = torch.tensor([labels.index(ch) for s in sents for ch in s], dtype=torch.int32)
    return torch.from_numpy(p).to(DEV), torch.from_numpy(sizes), targets, torch.tensor([len(s) for s in sents], dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def _both():
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.lm_search import LMGridSearch
    labels = _labels()
    batches = [_batch(21, 3, 17), _batch(22, 8, 40)]
    search = LMGridSearch(D.BeamCTCDecoder(labels, ARPA, **KW), POINTS)
    for b in batches:
        search.update(*b)
    want = []
    tgt = D.GreedyDecoder(labels)
    for alpha, beta in POINTS:
        dec = D.BeamCTCDecoder(labels, ARPA, alpha, beta, **KW)
        wer, cer = D.WordErrorRate(dec, tgt), D.CharErrorRate(dec, tgt)
        for b in batches:
            wer.update(*b)
            cer.update(*b)
        assert wer.total > 0 and cer.total > 0
        want.append([alpha, beta, wer.compute(), cer.compute()])
    return batches, search, want


def test_results_equal_the_loop_over_single_point_decoders():
    _, search, want = _both()
    assert search.char_err.is_cuda and search.char_err.dtype == torch.int64 and search.word_err.shape == (len(POINTS),)
    got = search.results()
    assert got == want
    assert got[2] == got[5] and len({tuple(r[2:]) for r in got}) > 1          # the points matter


def test_best_and_saved_json(tmp_path):
    _, search, want = _both()
    assert search.best() == min(want, key=lambda r: r[2]) and search.best("cer") == min(want, key=lambda r: r[3])
    path = str(tmp_path / "lm_search.json")
    search.save(path)
    with open(path) as f:
        assert json.load(f) == want


def test_decode_grid_strings_equal_decode_at_each_point():
    from deepspeech.pytorch_amd import decoder as D
    labels = _labels()
    (probs, sizes, _, _), _ = _both()[0]
    strings, offsets, scores = D.BeamCTCDecoder(labels, ARPA, **KW).decode_grid(probs, sizes, POINTS)
    assert len(strings) == len(POINTS) and scores.shape == (len(POINTS), 3) and not scores.is_cuda
    for g, (alpha, beta) in enumerate(POINTS):
        s, o, sc = D.BeamCTCDecoder(labels, ARPA, alpha, beta, **KW).decode_beams(probs, sizes)
        for n in range(3):
            assert strings[g][n] == s[n][0] and torch.equal(offsets[g][n], o[n][0]) and offsets[g][n].dtype == torch.int32
        assert torch.equal(scores[g].view(torch.int32), sc[:, 0].contiguous().view(torch.int32))
