"""Host checks (-m "not gpu") of the restatement that the hot-word GPU tests rely on (tests/beam_hot_reference.py): against brute
force over all paths with a plain-Python walk over the string, the state rules on hand-written cases, the equivalences with
the searches without hot words, and -- on the very inputs of the GPU grid (tests/beam_hot_cases.py) -- that every rule fires
and that the top beam is compared by rank in at least 90 % of the utterances."""
import math

import numpy as np
import pytest

import beam_hot_cases as HC
from beam_hot_reference import HOT, HotTable, beam_search_hot, walk
from beam_lm_reference import Scorer, beam_search_lm
from beam_reference import beam_search, brute_force

LABELS4 = ["_", "A", "N", " "]           # blank, two letters, space
SP = 3


def _probs(rng, T, C, scale=2.0):
    z = rng.standard_normal((T, C)) * scale
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def _ids(text, labels=LABELS4):
    return tuple(labels.index(ch) for ch in text)


# ---- brute force ----------------------------------------------------------------------------------------------------------------
def _plain_terms(m, text, phrases, alpha, beta, lexicon, oov_logp):
    """(lm term, hot_end) of a transcript by a walk over its characters that keeps the match as a text suffix; None when lexicon
    mode has no such beam.  phrases: {text: weight}.  Written on strings, apart from the restatement's tuples and tables."""
    prefixes = {ph[:k] for ph in phrases for k in range(1, len(ph) + 1)}
    val = lambda ph: float(np.float32(np.float64(np.float32(phrases[ph])) * len(ph.replace(' ', ''))))     # c of a whole phrase
    grams = None if m is None else {tuple(m.words[i] for i in ids): (float(p), float(b)) for d in m.ngrams for ids, (p, b) in d.items()}
    vocab = set() if m is None else {w for w in m.words if all(ch in LABELS4[1:3] for ch in w)}
    hist = [] if m is None else ["<s>"] * (m.order - 1)
    mu, part, done, lm = "", "", 0.0, 0.0

    def word_event(end):
        nonlocal lm
        known = part in vocab
        covered = mu in phrases or (not end and mu + " " in prefixes)
        ctx = tuple(hist[len(hist) - (m.order - 1):]) if m.order > 1 else ()
        if not known and covered:
            lnp, mark = float(np.float32(oov_logp)), "<hot>"
        elif not known or None in ctx:
            lnp, mark = -1000.0, None
        else:
            acc, mark = 0.0, part
            while ctx + (part,) not in grams:
                acc += grams[ctx][1] if ctx in grams else 0.0
                ctx = ctx[1:]
            lnp = (acc + grams[ctx + (part,)][0]) / math.log10(math.e)
        lm += alpha * lnp + beta
        hist.append(mark)
        return known or covered

    for ch in text:
        if ch != ' ':
            new = mu + ch if mu and mu + ch in prefixes else (part + ch if part + ch in prefixes else "")
            if m is not None and lexicon and not new and not any(v.startswith(part + ch) for v in vocab):
                return None
            mu, part = new, part + ch
            continue
        if m is not None:
            if not part:
                if lexicon:
                    return None
            elif not word_event(False) and lexicon:
                return None
        if mu in phrases:
            done, mu = done + val(mu), ""
        else:
            mu = mu + " " if mu and mu + " " in prefixes else ""
        part = ""
    if m is not None and part:
        word_event(True)
    return lm, done + (val(mu) if mu in phrases else 0.0)


@pytest.mark.parametrize("name,T,lexicon,alpha,beta", [
    (None, 5, False, 0.0, 0.0), ("toy5", 5, False, 0.9, 2.0), ("toy5", 5, True, 0.9, 2.0), ("toy1", 4, True, 0.7, 1.5),
    ("toy3", 5, False, 1.3, 0.5),
])
def test_wide_beam_equals_brute_force_plus_lm_and_hot_terms(name, T, lexicon, alpha, beta):
    # NN and NNA are outside every toy vocabulary (covered out-of-vocabulary words), AN and A are inside
    phrases = {"AN A": 1.25, "NN": 0.75, "NNA N": 2.0, "A": 0.5}
    table = HotTable([(_ids(ph), w) for ph, w in phrases.items()], SP)
    m = None if name is None else HC.lm(name)
    rng = np.random.default_rng(10 * T + len(name or ""))
    p = _probs(rng, T, 4)
    exact = brute_force(p)
    sc = None if m is None else Scorer(m, LABELS4, 0, alpha, beta, lexicon, np.float64)
    res = beam_search_hot(p, T, 0, 10 ** 6, 4, 1.0, table, sc, -11.5, np.float64)
    got = {lab: (s, a) for lab, _, s, a in res["beams"]}
    assert len(got) == len(res["beams"])
    a32, b32 = float(np.float32(alpha)), float(np.float32(beta))
    want = {}
    for lab, nll in exact.items():
        terms = _plain_terms(m, ''.join(LABELS4[c] for c in lab), phrases, a32, b32, lexicon, -11.5)
        if terms is not None:
            want[lab] = (nll - terms[0] - terms[1], nll)
    assert set(got) == set(want)
    if not (m is not None and lexicon):
        assert len(want) == len(exact) > 100             # every string that T frames can spell
    for lab, (s, a) in want.items():
        assert abs(got[lab][0] - s) <= 1e-9 * max(1.0, abs(s)), (lab, got[lab], s)
        assert abs(got[lab][1] - a) <= 1e-9 * max(1.0, abs(a)), (lab, got[lab], a)
    totals = [s for _, _, s, _ in res["beams"]]
    assert totals == sorted(totals)
    assert res["completions"] > 0 and res["fallbacks"] > 0
    if not lexicon:
        assert res["breaks"] > 0                           # a tiny lexicon drops most strings in which a match breaks
    if m is not None:
        assert res["covered_oov"] > 0
        assert lexicon == (res["lexicon_rescues"] > 0)
        # a covered out-of-vocabulary word costs hot_oov_logp, not -1000: "NN " is a beam whose lm term is small
        nn = _ids("NN ")
        assert nn in got and got[nn][0] - got[nn][1] < 50


# ---- the state rules, one hand-written case each ----------------------------------------------------------------------------------
def _table():
    lab = HC.labels()
    ph = [("NEW YORK", 2.0), ("THE CAT", 1.5), ("THE CAN", 2.5), ("TENT", 3.0)]
    return lab, HotTable([(_ids(t, lab), w) for t, w in ph], lab.index(' '))


def _walk(text, dtype=np.float32):
    lab, table = _table()
    mu, done, events = walk(table, _ids(text, lab), dtype)
    return (''.join(lab[c] for c in mu), float(done), events, float(table.hot(mu, done, np.float32)),
            float(table.hot_end(mu, done, np.float32)))


def test_state_walk_follows_every_rule():
    # a completion at a space: NEW YORK has 7 non-space labels at 2.0
    mu, done, ev, hot, end = _walk("NEW YORK ")
    assert (mu, done, hot, end) == ("", 14.0, 14.0, 14.0) and ev[-1] == "completion" and ev.count(None) == 8
    # a completion at the end: nothing is in done yet, hot_end pays the whole phrase
    assert _walk("NEW YORK")[:2] == ("NEW YORK", 0.0) and _walk("NEW YORK")[3:] == (14.0, 14.0)
    # an unfinished prefix earns nothing at the end, whatever it showed on the way
    assert _walk("NEW YO")[1:2] + _walk("NEW YO")[3:] == (0.0, 10.0, 0.0)
    # a break in mid-word
    mu, done, ev, hot, end = _walk("NEW YOX")
    assert (mu, done, hot, end) == ("", 0.0, 0.0, 0.0) and ev[-1] == "break"
    # NEW YORKER earns nothing: the match breaks at the E, and the space finds nothing to complete
    mu, done, ev, hot, end = _walk("NEW YORKER ")
    assert (mu, done, hot, end) == ("", 0.0, 0.0, 0.0) and ev[8] == "break" and "completion" not in ev
    # the fallback in NEW NEW YORK: "NEW N" is no prefix, "N" is one
    mu, done, ev, hot, end = _walk("NEW NEW YORK")
    assert ev[4] == "fallback" and (mu, done, end) == ("NEW YORK", 0.0, 14.0)
    assert _walk("NEW N")[0] == "N"
    # a double space ends the match
    mu, done, ev, hot, end = _walk("NEW  YORK")
    assert ev[4] == "break" and (mu, done, end) == ("", 0.0, 0.0)
    # a phrase at the very start and one after another word; a match starts at a word start only
    assert _walk("TENT ")[1] == 12.0 and _walk("A TENT ")[1] == 12.0 and _walk("ATENT ")[1] == 0.0
    assert _walk("TENT TENT NEW YORK")[1] == 24.0 and _walk("TENT TENT NEW YORK")[4] == 38.0
    # v is the maximum over the phrases that share the prefix: THE CA is worth 2.5 * 5, THE CAT 1.5 * 6
    assert _walk("THE CA")[3] == 12.5 and _walk("THE CAT")[3:] == (9.0, 9.0) and _walk("THE CAN ")[1] == 15.0


def test_fp32_sums_are_rounded_where_the_rules_say():
    lab = HC.labels()
    sp = lab.index(' ')
    w = 0.1                                                 # fp32(0.1) * 3 in fp64, rounded once: not fp32(0.1) * fp32(3) chained sums
    table = HotTable([(_ids("CAT", lab), w)], sp)
    c = table.c(_ids("CAT", lab))
    assert c.dtype == np.float32 and c == np.float32(np.float64(np.float32(w)) * 3)
    mu, done, _ = walk(table, _ids("CAT CAT CAT ", lab))
    assert done.dtype == np.float32 and done == np.float32(np.float32(c + c) + c)
    mu, done64, _ = walk(table, _ids("CAT CAT CAT ", lab), np.float64)
    assert done64 == float(c) * 3


# ---- equivalences: nothing else moved ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,top_n,cutoff", [(10 ** 6, 5, 1.0), (3, 5, 1.0), (8, 3, 0.9), (1, 5, 1.0)])
def test_zero_weights_equal_the_searches_without_hot_words(B, top_n, cutoff):
    m = HC.lm("toy3")
    labels = ["_", "A", "N", "D", " "]
    table = HotTable([(_ids(t, labels), 0.0) for t in ("AN AND", "AND", "A")], 4)       # every word is in toy3's vocabulary
    rng = np.random.default_rng(B % 1000 + top_n)
    for dtype in (np.float32, np.float64):
        for _ in range(4):
            p = _probs(rng, 12 if B < 100 else 6, 5)
            ref = beam_search(p, len(p), 0, B, top_n, cutoff, dtype=dtype)["beams"]
            got = beam_search_hot(p, len(p), 0, B, top_n, cutoff, table, None, dtype=dtype)["beams"]
            assert [(lab, fr, s) for lab, fr, s, _ in got] == ref and all(s == a for _, _, s, a in got)
            for lexicon in (False, True):
                sc = Scorer(m, labels, 0, 1.1, 0.4, lexicon, dtype)
                assert beam_search_hot(p, len(p), 0, B, top_n, cutoff, table, sc)["beams"] == \
                    beam_search_lm(p, len(p), 0, B, top_n, cutoff, sc)["beams"]


def test_hot_context_id_backs_off_with_backoff_zero():
    m = HC.lm("toy3")
    sc = Scorer(m, HC.labels(), 0, 1.0, 0.0, False, np.float64)
    the, cat = m.word_id["THE"], m.word_id["CAT"]
    uni = float(m.ngrams[0][(cat,)][0]) / math.log10(math.e)
    bi = float(m.ngrams[1][(the, cat)][0]) / math.log10(math.e)
    assert sc.ln_p(cat, (the, HOT)) == pytest.approx(uni, rel=1e-12)       # the newest word is the hot one: the unigram, no backoff
    assert sc.ln_p(cat, (HOT, the)) == pytest.approx(bi, rel=1e-12)        # an older one: the bigram, the trigram context adds 0
    assert sc.ln_p(cat, (the, -1)) == -1000.0                              # unlike the out-of-vocabulary mark


# ---- the GPU grid's inputs ------------------------------------------------------------------------------------------------------
def test_gpu_grid_fires_every_rule_and_compares_the_top_beam_by_rank():
    total = {k: 0 for k in HC.COUNTERS}
    lm_total = {k: 0 for k in HC.COUNTERS}
    compared = utterances = 0
    for c in HC.GRID:
        for ref in HC.case(*c)[2]:
            utterances += 1
            compared += len(ref["beams"]) > 0 and not HC.near(ref["beams"], 0)
            for k in HC.COUNTERS:
                total[k] += ref[k]
                if c[3] is None:
                    lm_total[k] += ref[k]
    assert all(v > 0 for v in total.values()), total
    assert all(lm_total[k] > 0 for k in ("completions", "breaks", "fallbacks")), lm_total       # without an LM too
    assert utterances == sum(c[0] for c in HC.GRID) and compared >= 0.9 * utterances, (compared, utterances)
    shapes = {(c[1], c[2]) for c in HC.GRID}
    assert {t for t, _ in shapes} == {0, 1, 2, 17, 60, 200} and {b for _, b in shapes} == {1, 2, 16, 256}
