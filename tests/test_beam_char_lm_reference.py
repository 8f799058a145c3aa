"""Host checks of the character-LM rules (DESIGN.md "ds2_beam", character language model): the numpy restatement
(tests/beam_char_lm_reference.py) against brute force, the plain restatement at zero weights, the <s> padding and the
out-of-vocabulary rule, and the host side of the feature: lm.char_ids / is_character_based / build_char_tables and the
lm_unit / space_token arguments of decoder.BeamCTCDecoder.  No GPU needed."""
import os

import numpy as np
import pytest

from beam_char_lm_reference import LOG10_E, OOV, OOV_SCORE, CharScorer, beam_search_clm
from beam_reference import beam_search, brute_force

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm")
CHAR_FILES = ["char1", "char3", "char5", "cjk3"]
CJK_LABELS = ["_"] + [chr(0x4E00 + i) for i in range(300)]


def _path(name):
    return os.path.join(GOLDEN, name + ".arpa")


def _lm(name):
    from deepspeech.pytorch_amd import lm
    return lm.load_arpa(_path(name))


def _labels():
    from deepspeech.pytorch_amd.configs import LABELS
    return list(LABELS)


def _softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("name,T,C", [("char3", 4, 4), ("char5", 5, 3), ("char1", 5, 4), ("char3", 3, 4)])
def test_fp64_form_equals_brute_force_plus_the_strings_own_bonuses(name, T, C):
    """nothing is pruned (B above the number of strings): every string's total is its exact -log p less its own sum of bonuses"""
    rng = np.random.default_rng(T * 10 + C)
    labels = ["_", "A", "T", "|"][:C]
    p = _softmax(rng.standard_normal((T, C)) * 2.0)
    sc = CharScorer(_lm(name), labels, 0, 1.3, 0.4, "|" if C == 4 else None, np.float64)
    bf = brute_force(p)
    got = beam_search_clm(p, T, 0, 4 ** 5, 40, 1.0, sc)["beams"]
    assert len(got) == len(bf) > 10
    worst = 0.0
    for lab, _, total, acoustic in got:
        lm, _ = sc.string_lm(lab)
        worst = max(worst, abs(total - (bf[lab] - float(lm))), abs(acoustic - bf[lab]))
    assert worst <= 1e-12, worst
    assert [g[2] for g in got] == sorted(g[2] for g in got)


@pytest.mark.parametrize("T,B,cutoff_prob", [(17, 10, 1.0), (61, 128, 0.9), (40, 256, 1.0)])
def test_zero_weights_equal_the_plain_restatement_exactly(T, B, cutoff_prob):
    rng = np.random.default_rng(T)
    p = _softmax(rng.standard_normal((T, 29)) * 3.0)
    plain = beam_search(p, T, 0, B, 40, cutoff_prob)["beams"]
    got = beam_search_clm(p, T, 0, B, 40, cutoff_prob, CharScorer(_lm("char3"), _labels(), 0, 0.0, 0.0, "|"))["beams"]
    assert [g[:3] for g in got] == plain and all(g[2] == g[3] for g in got)


def test_the_first_labels_see_s_in_front():
    """order 5: the first four labels have <s> ... <s> before them, the fifth a context of labels alone"""
    m = _lm("char5")
    sc = CharScorer(m, _labels(), 0, 1.0, 0.0, "|", np.float64)
    lab = [_labels().index(c) for c in "THE C"]
    ids = [sc.cid[c] for c in lab]
    assert ids[3] == m.word_id["|"] and OOV not in ids
    ctx, seen = sc.start, []
    for i in ids:
        seen.append(ctx)
        ctx = sc.shift(ctx, i)
    bos = m.bos
    assert seen == [(bos,) * 4, (bos,) * 3 + (ids[0],), (bos,) * 2 + tuple(ids[:2]), (bos,) + tuple(ids[:3]), tuple(ids[:4])]
    assert sc.string_lm(())[0] == 0.0 and sc.string_lm(())[1] == (bos,) * 4
    # "<s> T" is a stored bigram: the first label is scored from it after the backoffs of the longer contexts of <s>, which
    # are not stored and add 0
    hit = m.ngrams[1][(bos, ids[0])]
    assert sc.ln_p(ids[0], (bos,) * 4) == float(hit[0]) / LOG10_E
    total, _ = sc.string_lm(lab)
    assert abs(float(total) - sum(sc.ln_p(i, c) for i, c in zip(ids, seen))) < 1e-12


@pytest.mark.parametrize("name", ["char1", "char3", "char5"])
def test_an_unknown_label_poisons_the_next_order_minus_one_events_and_no_more(name):
    m = _lm(name)
    labels = _labels()
    sc = CharScorer(m, labels, 0, 1.0, 0.0, "|", np.float64)
    assert "Q" not in m.word_id and sc.cid[labels.index("Q")] == OOV
    lab = [labels.index(c) for c in "THEQ CAT SAT"]
    ctx, lnp = sc.start, []
    for c in lab:
        lnp.append(sc.ln_p(sc.cid[c], ctx))
        ctx = sc.shift(ctx, sc.cid[c])
    poisoned = [i for i, v in enumerate(lnp) if v == OOV_SCORE]
    assert poisoned == list(range(3, 3 + m.order))      # the Q itself and the order - 1 events that have it in their context
    assert all(v > -50 for i, v in enumerate(lnp) if i not in poisoned)


def test_space_token_given_absent_and_unknown():
    from deepspeech.pytorch_amd import lm
    m = _lm("char3")
    labels = _labels()
    sp = labels.index(" ")
    ids = lm.char_ids(m, labels, 0, "|")
    assert ids.dtype == np.int32 and ids.shape == (len(labels),)
    assert ids[sp] == m.word_id["|"] and ids[0] == -1 and ids[labels.index("T")] == m.word_id["T"]
    assert ids[labels.index("Q")] == -1 and (ids[1:] >= 0).sum() == len(m.words) - 3          # every unigram but the three marks
    none = lm.char_ids(m, labels, 0)
    assert none[sp] == -1 and (np.delete(none, sp) == np.delete(ids, sp)).all()
    with pytest.raises(ValueError, match="space_token"):
        lm.char_ids(m, labels, 0, "#")
    # the restatement looks its ids up on its own and agrees
    assert CharScorer(m, labels, 0, 1, 0, "|").cid == ids.tolist() and CharScorer(m, labels, 0, 1, 0).cid == none.tolist()
    with pytest.raises(ValueError):
        CharScorer(m, labels, 0, 1, 0, "#")
    # multi-byte labels, two-byte ids
    cj = lm.char_ids(_lm("cjk3"), CJK_LABELS, 0)
    assert cj[0] == -1 and (cj[1:] >= 3).all() and len(set(cj[1:].tolist())) == 300 and cj.max() > 255
    got_ids, table = lm.build_char_tables(m, labels, 0, "|")
    word_mode = lm.build_tables(m, labels, 0, sp)[1]
    assert (got_ids == ids).all() and (lm.build_char_tables(m, labels, 0, "|", spread=1)[1] == word_mode).all()
    assert table.shape == (lm.CHAR_TABLE_SPREAD * word_mode.shape[0], 2)                      # the same keys, spread out
    assert (table[:, 0] != -1).sum() == (word_mode[:, 0] != -1).sum() == sum(m.counts)
    for row, p, b in zip(m.ids[2], m.logp[2], m.backoff[2]):
        assert lm.ngram_lookup(table, lm.ngram_key(row.tolist())) == (p, b)


def test_is_character_based_and_auto():
    from deepspeech.pytorch_amd import lm
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    labels = _labels()
    for name in CHAR_FILES:
        assert lm.is_character_based(_lm(name))
    for name in ("toy1", "toy3", "toy5"):
        assert not lm.is_character_based(_lm(name))
        assert BeamCTCDecoder(labels, _path(name), lm_unit="auto").lm_unit == "word"
    for name in CHAR_FILES[:3]:
        dec = BeamCTCDecoder(labels, _path(name), lm_unit="auto", space_token="|")
        assert dec.lm_unit == "char"
        assert BeamCTCDecoder(labels, _path(name)).lm_unit == "word"                        # the default stays
    assert BeamCTCDecoder(CJK_LABELS, _path("cjk3"), lm_unit="auto").lm_unit == "char"         # no space label needed
    assert BeamCTCDecoder(CJK_LABELS, _path("cjk3"), lm_unit="char").space_index == len(CJK_LABELS)
    with pytest.raises(ValueError, match="space label"):
        BeamCTCDecoder(CJK_LABELS, _path("cjk3"))                                             # word mode still needs one
    with pytest.raises(ValueError, match="space_token"):
        BeamCTCDecoder(labels, _path("char3"), lm_unit="char", space_token="#")
    with pytest.raises(ValueError, match="lm_unit"):
        BeamCTCDecoder(labels, _path("char3"), lm_unit="syllable")
    assert BeamCTCDecoder(labels, lm_unit="char").lm_unit == "word" and BeamCTCDecoder(labels, lm_unit="char").lm is None


def test_hot_words_in_character_mode_are_refused():
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    labels = _labels()
    with pytest.raises(ValueError, match="hot words"):
        BeamCTCDecoder(labels, _path("char3"), lm_unit="char", space_token="|", hotwords=["THE CAT"])
    with pytest.raises(ValueError, match="hot words"):
        BeamCTCDecoder(labels, _path("char3"), lm_unit="auto", space_token="|", hotwords=["THE CAT"])
    dec = BeamCTCDecoder(labels, _path("char3"), lm_unit="char", space_token="|")
    with pytest.raises(ValueError, match="hot words"):
        dec.set_hotwords([("CAT", 3.0)])
    dec.set_hotwords(None)
    dec.set_hotwords([])
    assert dec.hotwords == []
    assert BeamCTCDecoder(labels, _path("char3"), hotwords=["THE CAT"]).hotwords == ["THE CAT"]    # word mode takes them


def test_word_mode_on_a_one_character_file_gives_todays_tables():
    """lm_unit="word" (the default) on a file of one-character unigrams: words of length 1, the tables of lm.build_tables"""
    from deepspeech.pytorch_amd import lm
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    labels = _labels()
    m = _lm("char3")
    dec = BeamCTCDecoder(labels, _path("char3"), 1.0, 1.0)
    assert dec.lm_unit == "word"
    wt, gt = lm.build_tables(m, labels, 0, labels.index(" "))
    assert lm.word_lookup(wt, lm.hash_labels([labels.index("T")])) == m.word_id["T"]
    assert lm.word_lookup(wt, lm.hash_labels([labels.index("T"), labels.index("H")])) == lm.WORD_ABSENT
    import torch
    args =dec._lm_args(torch.device("cpu"))
    assert set(args) == {"space", "word_table", "ngram_table", "order", "bos", "alpha", "beta", "lexicon"}
    assert (args["word_table"].numpy() == wt).all() and (args["ngram_table"].numpy() == gt).all()
    char = BeamCTCDecoder(labels, _path("char3"), 1.0, 1.0, lm_unit="char", space_token="|")._lm_args(torch.device("cpu"))
    assert char["unit"] == "char" and set(char) == {"unit", "label_ids", "ngram_table", "order", "bos", "alpha", "beta"}
    assert (char["label_ids"].numpy() == lm.char_ids(m, labels, 0, "|")).all()
    assert (char["ngram_table"].numpy() == lm.ngram_table(m, lm.CHAR_TABLE_SPREAD)).all()
