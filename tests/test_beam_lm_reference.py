"""Host checks (-m "not gpu") of the language-model side of the beam search: the ARPA parser and the table build of
deepspeech/pytorch_amd/lm.py, the backoff rule (every context sums to one), and the restatement the GPU tests rely on
(tests/beam_lm_reference.py) against brute force over all paths with a plain-Python scorer over s.split(' ')."""
import itertools
import math
import os

import numpy as np
import pytest

from beam_lm_reference import OOV, Scorer, beam_search_lm
from beam_reference import beam_search, brute_force
from deepspeech.pytorch_amd import lm as LM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm")
FIXTURES = {"toy1": 1, "toy3": 3, "toy5": 5}
PRINTED_DIGITS = 6                      # decimals of the fixtures' log10 values (tests/golden/make_beam_lm.py)


def _lm(name):
    return LM.load_arpa(os.path.join(GOLDEN, name + ".arpa"))


def _probs(rng, T, C, scale=2.0):
    z = rng.standard_normal((T, C)) * scale
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


# ---- ARPA parse ---------------------------------------------------------------------------------------------------------------
def test_arpa_parse_counts_ids_values():
    m = _lm("toy3")
    assert m.order == 3 and m.counts == [35, 97, 57] and [len(i) for i in m.ids] == m.counts
    assert m.words[:4] == ["<unk>", "<s>", "</s>", "THE"] and m.bos == 1 and m.word_id["IT'S"] > 2
    assert {"A", "AN", "AND", "ANT"} <= set(m.words)
    assert all(a.dtype == np.float32 for a in m.logp + m.backoff) and all(i.dtype == np.int32 for i in m.ids)
    # against an independent read of the text
    text = open(os.path.join(GOLDEN, "toy3.arpa")).read().split("\n")
    assert text[6] == "-2.679428\t<unk>" and m.ngrams[0][(0,)] == (np.float32(-2.679428), np.float32(0.0))
    assert m.ngrams[0][(1,)] == (np.float32(-99.0), np.float32(-0.648395))
    row = next(ln for ln in text if "\tTHE CAT\t" in ln).split("\t")
    assert m.ngrams[1][(m.word_id["THE"], m.word_id["CAT"])] == (np.float32(row[0]), np.float32(row[2]))
    tri = [ln for ln in text[text.index("\\3-grams:") + 1:] if ln and not ln.startswith("\\")]
    assert len(tri) == 57 and all(len(ln.split("\t")) == 2 for ln in tri)          # the highest order has no backoff column
    w = tri[0].split("\t")[1].split()
    assert m.ngrams[2][tuple(m.word_id[x] for x in w)] == (np.float32(tri[0].split("\t")[0]), np.float32(0.0))
    assert _lm("toy1").order == 1 and _lm("toy1").counts == [35]
    m5 = _lm("toy5")
    assert m5.order == 5 and len(m5.words) == 8 and set(m5.words[3:]) == {"A", "AN", "NA", "NAN", "ANNA"}


@pytest.mark.parametrize("content", [
    b"mmap lm http://kheafield.com/code format version 5\n\x00\x01\x02\xff\xfe",      # a KenLM binary's first bytes
    b"",
    b"\\data\\\nngram 1=2\n\n\\1-grams:\n-1.0\t<s>\n",                                  # truncated: an entry and \end\ missing
    b"\\data\\\nngram 1=1\n\n\\1-grams:\n-1.0\t<s>\n\n\\end\\\nngram",                  # fine
    b"\\data\\\nngram 1=1\nngram 2=1\n\n\\1-grams:\n-1.0\t<s>\n\n\\2-grams:\n-1.0\t<s> X\n\n\\end\\\n",   # X is no unigram
    b"\\data\\\nngram 1=1\n\n\\1-grams:\nabc\t<s>\n\n\\end\\\n",
    b"\\data\\\nngram 1=1\n\n\\1-grams:\n-1.0\tA\n\n\\end\\\n",                         # no <s>
    b"\\data\\\n" + b"".join(b"ngram %d=0\n" % k for k in range(1, 7)) + b"\n\\end\\\n",       # order 6
])
def test_arpa_parse_refuses_other_input(tmp_path, content):
    f = tmp_path / "x.arpa"
    f.write_bytes(content)
    if content.endswith(b"\\end\\\nngram"):
        assert LM.load_arpa(str(f)).words == ["<s>"]
        return
    with pytest.raises(ValueError, match="ARPA"):
        LM.load_arpa(str(f))


def test_missing_file_is_a_value_error(tmp_path):
    with pytest.raises(ValueError, match="ARPA"):
        LM.load_arpa(str(tmp_path / "nothing.arpa"))


# ---- backoff, independent of the scorer ---------------------------------------------------------------------------------------
def _p_backoff(grams, words, ctx):
    """P(word | ctx) over word strings by the textbook recursion, from {words tuple: (log10 p, log10 backoff)}"""
    g = ctx + (words,)
    if g in grams:
        return 10.0 ** grams[g][0]
    if not ctx:
        return 0.0
    return 10.0 ** (grams[ctx][1] if ctx in grams else 0.0) * _p_backoff(grams, words, ctx[1:])


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_every_context_sums_to_one(name):
    m = _lm(name)
    grams = {tuple(m.words[i] for i in ids): (float(p), float(b)) for d in m.ngrams for ids, (p, b) in d.items()}
    # one P(w | ctx) is a product of at most `order` stored values.  A value v carries the rounding to PRINTED_DIGITS decimals and
    # to fp32 (half an ulp of a value below 16 in magnitude; -99 is <s>, whose P is 1e-99 either way), so P is off by a factor of
    # at most 10^(order * err), and so is the sum over w of the P, whose exact value is 1
    err = 0.5 * 10.0 ** -PRINTED_DIGITS + 2.0 ** -21
    assert max(abs(p) for p, _ in grams.values() if p > -90) < 16 and max(abs(b) for _, b in grams.values()) < 16
    bound = 10.0 ** (m.order * err) - 1.0
    n = 0
    for k in range(m.order):
        for ctx in itertools.product(m.words, repeat=k):
            total = sum(_p_backoff(grams, w, ctx) for w in m.words)
            assert abs(total - 1.0) <= bound, (ctx, total, bound)
            n += 1
    assert n == sum(len(m.words) ** k for k in range(m.order))


# ---- restatement against brute force --------------------------------------------------------------------------------------------
def _plain_lm_term(m, text, alpha, beta, lexicon_words):
    """sum over the words of text.split(' ') of alpha * ln P(word | previous words) + beta, on word strings; None when
    lexicon_words is given and a word but the last is outside it (such a string is no beam in lexicon mode)"""
    grams = {tuple(m.words[i] for i in ids): (float(p), float(b)) for d in m.ngrams for ids, (p, b) in d.items()}
    hist, total = ["<s>"] * (m.order - 1), 0.0
    pieces = text.split(' ')
    for n, w in enumerate(pieces):
        if not w:
            if lexicon_words is not None and n + 1 < len(pieces):
                return None                                   # a space on an empty partial word
            continue
        known = (w,) in grams
        if lexicon_words is not None and n + 1 < len(pieces) and not known:
            return None
        ctx = tuple(hist[len(hist) - (m.order - 1):]) if m.order > 1 else ()
        if not known or any(h is None for h in ctx):
            lnp = -1000.0
        else:
            log10 = None
            acc = 0.0
            while log10 is None:
                if ctx + (w,) in grams:
                    log10 = acc + grams[ctx + (w,)][0]
                else:
                    acc += grams[ctx][1] if ctx in grams else 0.0
                    ctx = ctx[1:]
            lnp = log10 / math.log10(math.e)
        total += alpha * lnp + beta
        hist.append(w if known else None)
    return total


LABELS4 = ["_", "A", "N", " "]           # blank, two letters, space: A, AN, NA, NAN, ANNA can be spelled


@pytest.mark.parametrize("name,T,C,lexicon,alpha,beta", [
    ("toy1", 5, 4, False, 0.7, 1.5), ("toy1", 5, 4, True, 0.7, 1.5),
    ("toy3", 6, 4, False, 1.3, 0.5), ("toy3", 6, 4, True, 1.3, 0.5),
    ("toy5", 6, 4, False, 0.9, 2.0), ("toy5", 6, 4, True, 0.9, 2.0),
    ("toy3", 4, 3, False, 2.0, -1.0),
])
def test_wide_beam_equals_brute_force_plus_lm_term(name, T, C, lexicon, alpha, beta):
    m = _lm(name)
    labels = LABELS4 if C == 4 else ["_", "A", " "]
    rng = np.random.default_rng(100 * T + C + m.order)
    p = _probs(rng, T, C)
    exact = brute_force(p)
    sc = Scorer(m, labels, 0, alpha, beta, lexicon, np.float64)
    res = beam_search_lm(p, T, 0, 10 ** 6, C, 1.0, sc)
    got = {lab: (s, a) for lab, _, s, a in res["beams"]}
    assert len(got) == len(res["beams"])
    vocab = set(m.words) if lexicon else None
    spellable = [v for v in m.words if all(ch in labels[1:] for ch in v)]
    want = {}
    for lab, nll in exact.items():
        text = ''.join(labels[c] for c in lab)
        # in lexicon mode every partial word is a prefix of some vocabulary word that these labels spell
        if lexicon and any(not any(v.startswith(w) for v in spellable) for w in text.split(' ') if w):
            continue
        term = _plain_lm_term(m, text, float(np.float32(alpha)), float(np.float32(beta)), vocab)
        if term is not None:
            want[lab] = (nll - term, nll)
    assert set(got) == set(want)
    for lab, (s, a) in want.items():
        assert abs(got[lab][0] - s) <= 1e-9 * max(1.0, abs(s)), (lab, got[lab], s)
        assert abs(got[lab][1] - a) <= 1e-9 * max(1.0, abs(a)), (lab, got[lab], a)
    totals = [s for _, _, s, _ in res["beams"]]
    assert totals == sorted(totals)
    assert res["word_events"] > 0
    if not lexicon:
        assert res["oov_events"] > 0                          # e.g. "NN", or "AA" for the trigram
        oov = [lab for lab in want if any(w and w not in m.words for w in ''.join(labels[c] for c in lab).split(' '))]
        assert oov and all(want[lab][0] - want[lab][1] > 900 * alpha - 10 * abs(beta) for lab in oov)


@pytest.mark.parametrize("B,top_n,cutoff", [(10 ** 6, 5, 1.0), (3, 5, 1.0), (8, 3, 0.9), (1, 5, 1.0)])
def test_zero_weights_in_open_mode_equal_the_search_without_lm(B, top_n, cutoff):
    m = _lm("toy3")
    labels = ["_", "A", "N", "D", " "]
    rng = np.random.default_rng(B % 1000 + top_n)
    for dtype in (np.float32, np.float64):
        for _ in range(4):
            p = _probs(rng, 12 if B < 100 else 6, 5)
            ref = beam_search(p, len(p), 0, B, top_n, cutoff, dtype=dtype)["beams"]
            got = beam_search_lm(p, len(p), 0, B, top_n, cutoff, Scorer(m, labels, 0, 0.0, 0.0, False, dtype))["beams"]
            assert [(lab, fr, s) for lab, fr, s, _ in got] == ref
            assert all(s == a for _, _, s, a in got)


def test_scorer_counts_an_oov_context():
    m = _lm("toy3")
    sc = Scorer(m, ["_", "A", "N", "D", " "], 0, 1.0, 0.0, False, np.float64)
    a = m.word_id["A"]
    assert sc.ln_p(a, (m.bos, OOV)) == -1000.0 and sc.ln_p(OOV, (m.bos, m.bos)) == -1000.0
    assert sc.ln_p(a, (m.bos, m.bos)) == pytest.approx(float(m.ngrams[1][(m.bos, a)][0]) / math.log10(math.e), rel=1e-12)


# ---- table build ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_tables_hold_every_prefix_and_ngram(name):
    from deepspeech.pytorch_amd.configs import LABELS
    m = _lm(name)
    blank, space = 0, LABELS.index(' ')
    wt, gt = LM.build_tables(m, LABELS, blank, space)
    for t in (wt, gt):
        assert t.dtype == np.int64 and t.ndim == 2 and t.shape[1] == 2 and t.shape[0] & (t.shape[0] - 1) == 0
    spelled = [w for w in m.words if all(ch in LABELS for ch in w)]
    assert len(spelled) == len(m.words) - 3                  # all but <unk>, <s>, </s>
    prefixes = {w[:n] for w in spelled for n in range(1, len(w) + 1)}
    assert 2 * len(prefixes) <= len(wt) and 2 * sum(m.counts) <= len(gt)
    assert int((wt.view(np.uint64)[:, 0] != LM.EMPTY_KEY).sum()) == len(prefixes)
    assert int((gt.view(np.uint64)[:, 0] != LM.EMPTY_KEY).sum()) == sum(m.counts)
    for pre in prefixes:
        v = LM.word_lookup(wt, LM.hash_labels([LABELS.index(ch) for ch in pre]))
        assert v == (m.word_id[pre] if pre in m.word_id else LM.WORD_PREFIX), pre
    for absent in ("Q", "THEX", "CATS", "ZZ", "AX"):
        assert LM.word_lookup(wt, LM.hash_labels([LABELS.index(ch) for ch in absent])) == LM.WORD_ABSENT
    assert LM.word_lookup(wt, LM.HASH_EMPTY) == LM.WORD_ABSENT
    for d in m.ngrams:
        for ids, (p, b) in d.items():
            assert LM.ngram_lookup(gt, LM.ngram_key(ids)) == (p, b), ids
    V = len(m.words)
    rng = np.random.default_rng(1)
    missed = 0
    for _ in range(300):
        ids = tuple(int(v) for v in rng.integers(0, V, size=int(rng.integers(1, m.order + 2))))
        if len(ids) > m.order or ids not in m.ngrams[len(ids) - 1]:
            assert LM.ngram_lookup(gt, LM.ngram_key(ids)) is None
            missed += 1
    assert missed > 50
    assert LM.ngram_key((3, 4)) != LM.ngram_key((4, 3)) and LM.ngram_key((3,)) != LM.ngram_key((3, 0))


def test_an_engineered_key_collision_raises(monkeypatch):
    with pytest.raises(ValueError, match="same hash key"):
        LM.make_table(np.array([5, 9, 5], np.uint64), np.array([1, 2, 3]))
    with pytest.raises(ValueError, match="free-slot"):
        LM.make_table(np.array([LM.EMPTY_KEY], np.uint64), np.array([1]))
    from deepspeech.pytorch_amd.configs import LABELS
    m = _lm("toy3")
    monkeypatch.setattr(LM, "NGRAM_MUL", 0)                    # every id tuple gets one key
    with pytest.raises(ValueError, match="n-gram table.*same hash key"):
        LM.build_tables(m, LABELS, 0, LABELS.index(' '))
    monkeypatch.undo()
    monkeypatch.setattr(LM, "HASH_BASE", 1)                    # a string's hash is the sum of its labels: AN = NA
    m5 = _lm("toy5")
    with pytest.raises(ValueError, match="word table.*same hash key"):
        LM.build_tables(m5, LABELS, 0, LABELS.index(' '))


def test_table_probing_wraps_and_fills_to_half():
    keys = (np.arange(1, 65, dtype=np.uint64) << np.uint64(32)) | np.uint64(127)      # all start at the last slots
    t = LM.make_table(keys, np.arange(64))
    assert len(t) == 128
    assert all(LM.table_find(t, int(k)) == i for i, k in enumerate(keys))
    assert LM.table_find(t, 126) is None


def test_decoder_constructor_with_a_language_model():
    from deepspeech.pytorch_amd.configs import LABELS
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    path = os.path.join(GOLDEN, "toy3.arpa")
    dec = BeamCTCDecoder(LABELS, path, 1.5, 0.5, 40, 1.0, 16, 4, 0)              # the reference's positional order
    assert dec.lm.order == 3 and dec.alpha == 1.5 and dec.beta == 0.5 and dec.beam_width == 16 and dec.lexicon is True
    assert BeamCTCDecoder(LABELS, lm_path=path, lexicon=False).lexicon is False
    with pytest.raises(ValueError, match="space label"):
        BeamCTCDecoder(["_", "A", "B"], lm_path=path)
    with pytest.raises(ValueError, match="ARPA"):
        BeamCTCDecoder(LABELS, lm_path=__file__)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_scoring_through_the_tables_equals_scoring_through_the_dicts(name):
    """the kernel's way to a word bonus, on the host: keys of all suffixes from one pass over (word, newest context word, ...),
    table lookups, the longest hit plus the backoffs of the dropped contexts -- against Scorer.bonus (fp32: equal bits)"""
    from deepspeech.pytorch_amd.configs import LABELS
    m = _lm(name)
    _, gt = LM.build_tables(m, LABELS, 0, LABELS.index(' '))
    sc = Scorer(m, LABELS, 0, 1.3, 0.7, False, np.float32)
    alpha, beta = float(np.float32(1.3)), float(np.float32(0.7))
    rng = np.random.default_rng(2)
    for _ in range(2000):
        w = int(rng.integers(0, len(m.words)))
        ctx = tuple(int(v) for v in rng.integers(0, len(m.words), size=m.order - 1))       # oldest first
        h, g, pk, bk = LM.ngram_mix(LM.NGRAM_SEED, w), LM.NGRAM_SEED, [], []
        pk.append(h)
        for c in reversed(ctx):
            h, g = LM.ngram_mix(h, c), LM.ngram_mix(g, c)
            pk.append(h)
            bk.append(g)
        acc, hit = 0.0, False
        for k in range(m.order - 1, -1, -1):
            e = LM.ngram_lookup(gt, pk[k])
            if e is not None:
                acc += float(e[0])
                hit = True
                break
            b = LM.ngram_lookup(gt, bk[k - 1])
            acc += float(b[1]) if b is not None else 0.0
        assert hit
        assert np.float32(alpha * (acc / LM.LOG10_E) + beta) == sc.bonus(w, ctx), (w, ctx)
