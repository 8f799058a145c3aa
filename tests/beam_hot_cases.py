"""The inputs that the hot-word tests share (tests/test_beam_hot_reference.py on the CPU, tests/test_gpu_beam_hot*.py on the
device): planted sentences as peaky rows with noise, then random rows, built as tests/test_gpu_beam_lm.py builds them.  The
sentences contain the hot phrases, near misses of them (NEW YORKER, NEW NEW YORK) and a phrase that the toy language models do
not know (NEW YORK; NANA for toy5).  Nothing here needs a GPU; the restatement's results are made once per case and shared."""
import functools
import os

import numpy as np

from beam_hot_reference import HotTable, beam_search_hot
from beam_lm_reference import Scorer

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm")
HOT_OOV_LOGP = -11.5
SENTENCES = {
    "toy3": ["THE CAT SAT ON THE MAT", "NEW YORK IS BIG", "HE SAW NEW YORKER", "NEW NEW YORK", "THEY SAT IN THE TENT",
             "A RED HAT", "THE CAN", "NEW  YORK"],
    "toy5": ["ANNA NAN A", "NANA AN", "AN ANNA NA", "NA NANAN", "ANNA ANNA NAN"],
}
SENTENCES["toy1"] = SENTENCES[None] = SENTENCES["toy3"]
PHRASES = {
    "toy3": ["NEW YORK", ("THE CAT", 1.5), ("THE CAN", 2.5), ("TENT", 3.0), "RED HAT"],
    "toy5": ["ANNA NAN", ("NANA", 3.0), ("NA", 1.0)],
}
PHRASES["toy1"] = PHRASES[None] = PHRASES["toy3"]
DEFAULT_WEIGHT = 2.0


def labels():
    from deepspeech.pytorch_amd.configs import LABELS
    return LABELS


@functools.lru_cache(maxsize=None)
def lm(name):
    from deepspeech.pytorch_amd import lm as LM
    return LM.load_arpa(os.path.join(GOLDEN, name + ".arpa"))


def hot_table(phrases, weight=None):
    """the restatement's table of `phrases`; weight: every phrase gets this one (0.0 for the equivalence tests)"""
    lab = labels()
    out = []
    for item in phrases:
        text, w = (item, DEFAULT_WEIGHT) if isinstance(item, str) else item
        out.append((tuple(lab.index(ch) for ch in text), w if weight is None else weight))
    return HotTable(out, lab.index(' '))


def _softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def planted(rng, T, sents, lab, peak=5.0, noise=1.5):
    """(T, C) probabilities: sentences drawn from sents, their labels one or two frames each (a blank between equal neighbours and
    after some labels) as peaky rows with noise over the first nine tenths of the frames, then random peaky rows"""
    path, prev = [], -1
    while len(path) < 0.9 * T:
        for ch in sents[int(rng.integers(0, len(sents)))] + " ":
            c = lab.index(ch)
            if c == prev or rng.random() < 0.3:
                path.append(0)
            path += [c] * int(rng.integers(1, 3))
            prev = c
    z = rng.standard_normal((T, len(lab))) * 3.0
    n = min(T, len(path), max(int(0.9 * T), 2))
    z[:n] = rng.standard_normal((n, len(lab))) * noise
    z[np.arange(n), path[:n]] += peak
    return _softmax(z)


def inputs(seed, N, T, name):
    rng = np.random.default_rng(seed)
    lab = labels()
    if T == 0:
        return np.zeros((N, 0, len(lab)), np.float32), np.zeros(N, np.int32)
    p = np.stack([planted(rng, T, SENTENCES[name] if T > 2 else ["N"], lab) for _ in range(N)])
    sizes = rng.integers(1, T + 1, size=N)
    sizes[0] = T
    if N >= 3:
        sizes[1] = 0
    return p, sizes.astype(np.int32)


# (N, T, B, model or None, lexicon, cutoff_top_n, cutoff_prob, strided (T, N, C) view, alpha, beta)
GRID = [
    (1, 0, 16, None, False, 40, 1.0, False, 0.0, 0.0),
    (3, 1, 2, None, False, 40, 1.0, False, 0.0, 0.0),
    (3, 2, 256, "toy3", True, 40, 1.0, False, 1.0, 1.0),
    (3, 17, 16, None, False, 40, 1.0, True, 0.0, 0.0),
    (3, 17, 1, "toy3", False, 40, 1.0, False, 1.2, 0.8),
    (2, 17, 256, "toy5", True, 3, 1.0, False, 0.8, 1.5),
    (3, 60, 16, "toy3", True, 40, 1.0, False, 1.2, 0.8),
    (3, 60, 256, "toy3", False, 40, 0.9, False, 1.0, 1.0),
    (3, 60, 2, None, False, 4, 1.0, False, 0.0, 0.0),
    (2, 60, 256, None, False, 40, 1.0, False, 0.0, 0.0),
    (3, 60, 16, "toy1", False, 40, 1.0, True, 1.5, 0.5),
    (3, 60, 16, "toy5", False, 40, 1.0, False, 0.5, 2.0),
    (2, 60, 16, "toy5", True, 40, 1.0, False, 0.9, 1.1),
    (1, 200, 16, "toy3", True, 40, 1.0, False, 1.1, 0.3),
]
COUNTERS = ("completions", "breaks", "fallbacks", "covered_oov", "lexicon_rescues")


def scorer(name, alpha, beta, lexicon, dtype=np.float32):
    return None if name is None else Scorer(lm(name), labels(), 0, alpha, beta, lexicon, dtype)


@functools.lru_cache(maxsize=None)
def case(N, T, B, name, lexicon, top_n, cutoff_prob, strided, alpha, beta):
    """the case's inputs and the restatement's result per utterance (made once, on the CPU)"""
    p, sizes = inputs(N * 1000 + T * 7 + B, N, T, name)
    table = hot_table(PHRASES[name])
    sc = scorer(name, alpha, beta, lexicon)
    refs = [beam_search_hot(p[n], sizes[n], 0, B, top_n, cutoff_prob, table, sc, HOT_OOV_LOGP) for n in range(N)]
    return p, sizes, refs


def near(rb, b):
    """whether beam b's total is within 1e-6 (relative) of a neighbour's: its rank is then not compared"""
    return (b > 0 and rb[b][2] - rb[b - 1][2] <= 1e-6 * max(1.0, abs(rb[b][2]))) or \
        (b + 1 < len(rb) and rb[b + 1][2] - rb[b][2] <= 1e-6 * max(1.0, abs(rb[b][2])))
