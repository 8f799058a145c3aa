"""Host checks (-m "not gpu") of deepspeech/pytorch_amd/hotwords.py: the phrase rules and their ValueErrors, the values of the
table (against the restatement's dict), the single rounding of the weights, the collision check, and the decoder's constructor
surface for hot words."""
import numpy as np
import pytest

import beam_hot_cases as HC
from deepspeech.pytorch_amd import hotwords as HW
from deepspeech.pytorch_amd import lm as LM


def _ids(text):
    lab = HC.labels()
    return tuple(lab.index(ch) for ch in text)


@pytest.mark.parametrize("phrases,match", [
    (["NEW YORK", "NEW YORK"], "'NEW YORK' is listed twice"),
    (["NEW YORK", ("NEW YORK", 3.0)], "'NEW YORK' is listed twice"),
    (["NEW YORK", "NEW YORK CITY"], "'NEW YORK' followed by a space is a prefix of 'NEW YORK CITY'.*'CITY' as a phrase of its own"),
    ([("TENT", -1.0)], "'TENT'.*weight"),
    ([("TENT", float("nan"))], "'TENT'.*weight"),
    ([("TENT", float("inf"))], "'TENT'.*weight"),
    ([("TENT", 1e39)], "'TENT'.*weight"),
    ([("TENT", "heavy")], "'TENT'.*weight"),
    ([""], "'' is empty"),
    ([" TENT"], "' TENT' starts or ends with a space"),
    (["TENT "], "'TENT ' starts or ends with a space"),
    (["NEW  YORK"], "'NEW  YORK' contains a double space"),
    (["NEW_YORK"], "'NEW_YORK' contains '_'"),                       # the blank
    (["new york"], "'new york' contains 'n'"),                       # no label
    ([("TENT", 1e38), "A"], "'TENT'.*no finite fp32"),               # 1e38 * 4 overflows fp32
    ([7], "string or a"),
])
def test_every_rule_raises_and_names_the_phrase(phrases, match):
    with pytest.raises(ValueError, match=match):
        HW.build_table(phrases, HC.labels(), 0)


def test_labels_need_a_space_other_than_the_blank():
    with pytest.raises(ValueError, match="space label"):
        HW.build_table(["AB"], ["_", "A", "B"], 0)
    with pytest.raises(ValueError, match="space label"):
        HW.build_table(["AB"], [" ", "A", "B"], 0)


def test_table_holds_every_prefix_with_the_restatements_values():
    lab = HC.labels()
    for name in ("toy3", "toy5"):
        phrases = HC.PHRASES[name]
        t = HW.build_table(phrases, lab, 0, HC.DEFAULT_WEIGHT)
        ref = HC.hot_table(phrases).entries
        assert t.dtype == np.int64 and t.ndim == 2 and t.shape[1] == 2 and t.shape[0] & (t.shape[0] - 1) == 0
        assert 2 * len(ref) <= len(t) and int((t.view(np.uint64)[:, 0] != LM.EMPTY_KEY).sum()) == len(ref)
        assert any(q[-1] == lab.index(' ') for q in ref)                     # prefixes that end in a space are entries too
        for q, (v, complete, c) in ref.items():
            got = HW.lookup(t, LM.hash_labels(q))
            assert got is not None and got[0].view(np.uint32) == v.view(np.uint32) and got[1] == complete, q
            assert got[2].view(np.uint32) == c.view(np.uint32), q
        for absent in ("X", "NEW X", "NEW YORKE", "TENTS", "NEW  "):
            assert HW.lookup(t, LM.hash_labels(_ids(absent))) is None
        assert HW.lookup(t, LM.HASH_EMPTY) is None


def test_v_is_the_maximum_over_the_phrases_sharing_a_prefix():
    pre = HW.prefix_values([("THE CAT", 1.5), ("THE CAN", 2.5), ("THEY", 4.0)], HC.labels(), 0)
    assert pre[_ids("THE CA")] == (np.float32(12.5), False, np.float32(0))
    assert pre[_ids("THE CAT")] == (np.float32(9.0), True, np.float32(9.0))
    assert pre[_ids("THE")] == (np.float32(12.0), False, np.float32(0))       # 4.0 * 3 beats 2.5 * 3
    assert pre[_ids("THEY")] == (np.float32(16.0), True, np.float32(16.0))
    assert pre[_ids("TH")] == (np.float32(8.0), False, np.float32(0))
    assert pre[_ids("THE ")] == (np.float32(7.5), False, np.float32(0))       # the space adds no label: n stays 3
    # a string takes the default weight, a pair its own
    pre = HW.prefix_values(["AB", ("CD", 0.0)], HC.labels(), 0, 0.75)
    assert pre[_ids("AB")] == (np.float32(1.5), True, np.float32(1.5)) and pre[_ids("CD")] == (np.float32(0), True, np.float32(0))


def test_weights_are_rounded_once():
    w = 0.1
    pre = HW.prefix_values([("ABCDEFG", w)], HC.labels(), 0)
    w32 = np.float32(w)
    chained = np.float32(0)
    for n in range(1, 8):
        chained = np.float32(chained + w32)
        once = np.float32(np.float64(w32) * n)
        assert pre[_ids("ABCDEFG"[:n])][0].view(np.uint32) == once.view(np.uint32)
    assert chained != np.float32(np.float64(w32) * 7)                         # the chained fp32 sum differs: it is not what is stored


def test_a_forged_collision_raises(monkeypatch):
    monkeypatch.setattr(LM, "HASH_BASE", 1)                    # a string's hash is the sum of its labels: AN = NA
    with pytest.raises(ValueError, match="hot-word table.*same hash key"):
        HW.build_table(["AN", "NA"], HC.labels(), 0)
    monkeypatch.undo()
    monkeypatch.setattr(LM, "hash_labels", lambda q: LM.HASH_EMPTY)            # a prefix with the empty string's hash
    with pytest.raises(ValueError, match="hot-word table.*same hash key"):
        HW.build_table(["A"], HC.labels(), 0)


def test_decoder_constructor_and_set_hotwords():
    import os
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    from deepspeech.pytorch_amd.lm_search import LMGridSearch
    lab = HC.labels()
    dec = BeamCTCDecoder(lab)
    assert dec.hotwords == [] and dec._hot_host is None and dec.hotword_weight == 2.0 and dec.hot_oov_logp == -11.5
    assert BeamCTCDecoder(lab, hotwords=[])._hot_host is None
    path = os.path.join(HC.GOLDEN, "toy3.arpa")
    dec = BeamCTCDecoder(lab, lm_path=path, hotwords=["ANNA KOWALSKI", ("TENT", 3.0)], hotword_weight=1.0)
    pre = HW.prefix_values(dec.hotwords, lab, 0, 1.0)
    assert pre[_ids("ANNA KOWALSKI")][2] == np.float32(12.0) and pre[_ids("TENT")][2] == np.float32(12.0)
    assert np.array_equal(dec._hot_host, HW.build_table(["ANNA KOWALSKI", ("TENT", 3.0)], lab, 0, 1.0))
    with pytest.raises(ValueError, match="hot words"):
        dec.decode_grid(None, None, [(1.0, 1.0)])
    with pytest.raises(ValueError, match="hot words"):
        dec.decode_grid_device(None, None, [(1.0, 1.0)])
    with pytest.raises(ValueError, match="hot words"):
        LMGridSearch(dec, [(1.0, 1.0)])
    dec.set_hotwords(None)
    assert dec.hotwords == [] and dec._hot_host is None
    LMGridSearch(dec, [(1.0, 1.0)])
    with pytest.raises(ValueError, match="'NEW  YORK'"):
        dec.set_hotwords(["NEW  YORK"])
    with pytest.raises(ValueError, match="space label"):
        BeamCTCDecoder(["_", "A", "B"], hotwords=["AB"])
    with pytest.raises(ValueError, match="hot_oov_logp"):
        BeamCTCDecoder(lab, hot_oov_logp=float("-inf"))
