"""Host checks of keyword spotting (run with -m "not gpu"): the numpy restatement of the rule (tests/kws_reference.py) against a
brute-force enumeration of every window and every path, its chunk-invariance, the packing of keywords into waves, the argument
checks of KeywordSpotter, and that header and binding name the same entry points."""
import itertools
import os
import re

import numpy as np
import pytest

import kws_reference as ref
from deepspeech.pytorch_amd import keywords as kwm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
LABELS = "_ABCDEFGH "          # index 0 is the blank


def ids_of(word):
    return [LABELS.index(c) for c in word]


def collapse(path, blank=0):
    out, prev = [], None
    for p in path:
        if p != prev and p != blank:
            out.append(p)
        prev = p
    return out


def brute_end_scores(r, ids, blank=0):
    """per end frame e: (the best score of a labelling of a window [a, e] that starts with y_1, ends with y_L, holds no other
    leading or trailing blank and collapses to the keyword, the set of starts a that reach it); (-inf, {}) when there is none"""
    T, C = r.shape
    out = []
    for e in range(T):
        best, starts = ref.NINF, set()
        for a in range(e + 1):
            for path in itertools.product(range(C), repeat=e - a + 1):
                if path[0] != ids[0] or path[-1] != ids[-1] or collapse(path, blank) != list(ids):
                    continue
                s = F32(0)
                for t, c in zip(range(a, e + 1), path):
                    s = F32(s + r[t, c])
                if s > best:
                    best, starts = s, {a}
                elif s == best:
                    starts.add(a)
        out.append((best, starts))
    return out


@pytest.mark.parametrize("word", ["A", "AB", "AA", "ABA", "AAB", "ABC"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_equals_brute_force(word, seed):
    rng = np.random.default_rng(seed)
    T, C = 6, 4
    # multiples of 1/8, few distinct values: ties are common and every sum is exact
    x = (rng.integers(-6, 1, size=(T, C)) / 8.0).astype(F32)
    r = ref.frame_scores(x, "log_probs")
    ids = ids_of(word)
    brute = brute_end_scores(r, ids)
    kw = ref.RefKeyword(ids, 0, F32(-100))
    best = (ref.NINF, -1, -1)
    for t in range(T):
        s, b = kw.step(r[t], t)
        assert s == brute[t][0], (t, s, brute[t])
        if s == ref.NINF:
            assert b == -1
        else:
            assert b in brute[t][1], (t, b, brute[t])
        if s > best[0]:
            best = (s, b, t)
    st = ref.RefStream([ids], [-100.0], 0)
    st.feed(x)
    assert st.best[0] == best
    top = max(s for s, _ in brute)
    assert best[0] == top and best[2] == [s for s, _ in brute].index(top)


def test_ties_keep_the_first_frame_and_extend_through_the_last_label():
    # A A A _ B B: every path through "AB" on its own frames scores 0
    x = np.full((8, 4), -4, F32)
    for t, c in enumerate([3, 1, 1, 1, 0, 2, 2, 3]):
        x[t, c] = 0
    hits, best, dropped = ref.spot(x, [ids_of("AB")], [-0.5], 0, hold=2)
    assert hits == [(0, 1, 6, F32(0))] and dropped == 0       # the run of A keeps its first frame, the hit runs through both B
    assert best == [(F32(0), 1, 5)]                            # best is replaced only when strictly greater: the first B
    # "AA" needs the blank between: A A alone is one A
    x = np.full((6, 4), -4, F32)
    for t, c in enumerate([1, 1, 0, 1, 1, 3]):
        x[t, c] = 0
    hits, best, _ = ref.spot(x, [ids_of("AA")], [-0.5], 0, hold=2)
    assert hits == [(0, 0, 4, F32(0))]
    x[2, 0], x[2, 1] = -4, 0                                   # without the blank frame: A A A A A, no "AA" at score 0
    hits, best, _ = ref.spot(x, [ids_of("AA")], [-0.5], 0, hold=2)
    assert hits == [] and best[0][0] == F32(-4)


def planted(T=200, C=10, seed=3):
    """the winner of every frame is at 0, the rest <= -1; "CDC" as C C _ D C C at 50..55 and "GGH" as G _ G H H at 120..124;
    elsewhere the winner is the blank, E or F, which neither keyword holds"""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-96, -7, size=(T, C)) / 8.0).astype(F32)
    win = rng.choice([0, 5, 6], size=T)
    win[50:56] = ids_of("CC_DCC")
    win[120:125] = ids_of("G_GHH")
    x[np.arange(T), win] = 0
    return x


def test_planted_occurrences_and_chunk_invariance():
    x = planted()
    kws, thr = [ids_of("CDC"), ids_of("GGH")], [-0.5, -0.5]
    hits, best, dropped = ref.spot(x, kws, thr, 0, hold=25, max_hits=8)
    assert hits == [(0, 50, 55, F32(0)), (1, 120, 124, F32(0))] and dropped == 0
    assert best == [(F32(0), 50, 54), (F32(0), 120, 123)]
    st = ref.RefStream(kws, thr, 0, hold=25, max_hits=8)
    got, at, pos = [], [], 0
    for i, n in enumerate([1, 7, 64, 0, 65, 63]):
        h = st.feed(x[pos:pos + n], end=i == 5)
        pos += n
        got += h
        at += [i] * len(h)
    assert pos == 200 and sorted(got) == sorted(hits) and st.best == best
    assert at == [4, 5]                 # CDC ends at 55 and its hold runs out at 80, in the chunk of 65 (frames 72..136); GGH at the end


@pytest.mark.parametrize("seed", [0, 1])
def test_chunk_invariance_on_noise(seed):
    rng = np.random.default_rng(seed)
    x = ref.grid_log_probs(rng, 90, 5)
    kws = [ids_of(w) for w in ["A", "AB", "ABBA", "DCBA", "AAAA"]]
    thr = [-12.0] * len(kws)                                   # every reachable frame qualifies: the merge rule works on noise
    for hold in (1, 3, 200):
        hits, best, _ = ref.spot(x, kws, thr, 0, hold=hold, max_hits=1000)
        st = ref.RefStream(kws, thr, 0, hold=hold, max_hits=1000)
        got, pos = [], 0
        for n in [1, 7, 0, 30, 2, 50]:
            got += st.feed(x[pos:pos + n])
            pos += n
        got += st.feed(x[:0], end=True)
        assert sorted(got) == sorted(hits) and st.best == best and st.frames == 90
        if hold == 1:
            assert len(hits) > len(kws)


def test_max_hits_counts_what_it_drops():
    x = ref.grid_log_probs(np.random.default_rng(5), 40, 4)
    full, _, d0 = ref.spot(x, [ids_of("A")], [-12.0], 0, hold=1, max_hits=1000)
    one, _, d1 = ref.spot(x, [ids_of("A")], [-12.0], 0, hold=1, max_hits=1)
    assert d0 == 0 and len(full) > 1 and one == full[:1] and d1 == len(full) - 1


@pytest.mark.parametrize("lengths, waves, where", [
    ([64], 1, [(0, 0)]),
    ([32, 32], 1, [(0, 0), (0, 32)]),
    ([33, 32], 2, [(0, 0), (1, 0)]),
    ([1] * 64, 1, [(0, i) for i in range(64)]),
    ([1] * 65, 2, [(0, i) for i in range(64)] + [(1, 0)]),
    ([63, 1, 1], 2, [(0, 0), (0, 63), (1, 0)]),
])
def test_packing(lengths, waves, where):
    assert kwm.pack_waves(lengths) == (where, waves)
    ids = [tuple(1 + (i + k) % 8 for i in range(L)) for k, L in enumerate(lengths)]
    lanes = kwm.pack(ids, [-1.0] * len(ids))
    assert lanes.shape == (waves * 64, 4) and lanes.dtype == np.int32
    seen = np.zeros(waves * 64, bool)
    for k, (L, (w, l0)) in enumerate(zip(lengths, where)):
        assert l0 + L <= 64                                    # none straddles a wave
        rows = lanes[w * 64 + l0:w * 64 + l0 + L]
        assert rows[:, 0].tolist() == list(ids[k]) and (rows[:, 2] == k).all()
        assert [bool(f & kwm.FIRST) for f in rows[:, 1]] == [i == 0 for i in range(L)]
        assert [bool(f & kwm.LAST) for f in rows[:, 1]] == [i == L - 1 for i in range(L)]
        assert [bool(f & kwm.SKIP) for f in rows[:, 1]] == [i > 0 and ids[k][i] != ids[k][i - 1] for i in range(L)]
        assert (rows[:, 3].view(np.float32) == np.float32(-1.0 * L)).all()
        seen[w * 64 + l0:w * 64 + l0 + L] = True
    assert (lanes[~seen] == (-1, 0, -1, 0)).all()


def test_pack_flags_repeats():
    lanes = kwm.pack([(1, 1, 2)], [-0.3])
    assert lanes[:3, 1].tolist() == [kwm.FIRST, 0, kwm.SKIP | kwm.LAST]
    assert lanes[0, 3].view(np.float32) == np.float32(np.float64(-0.3) * 3)


@pytest.mark.parametrize("keywords, what", [
    ([""], "is empty"),
    (["AB_"], "'AB_' contains '_'"),
    (["ABZ"], "'ABZ' contains 'Z'"),
    (["A" * 65], "has 65 labels"),
    (["AB", "C", "AB"], "'AB' is listed twice"),
    ([("AB", 0.5)], "'AB': the threshold"),
    ([("AB", "x")], "'AB': the threshold"),
    ([3], "a keyword is a string"),
    ([], "at least one keyword"),
])
def test_validation_names_the_keyword(keywords, what):
    with pytest.raises(ValueError, match=re.escape(what)):
        kwm.KeywordSpotter(LABELS, keywords)


def test_spotter_arguments():
    sp = kwm.KeywordSpotter(LABELS, [" A ", ("AB", -0.25)], hold=3, frame_seconds=0.02)
    assert sp.label_ids == [(9, 1, 9), (1, 2)] and sp.thresholds == [-1.0, -0.25]       # the space may stand first and last
    d = sp.detection(1, 5, 9, -0.25)
    assert d == kwm.Detection("AB", 1, 5, 9, -0.25, -0.125, 0.1, 0.2)
    for bad in (dict(hold=0), dict(hold=1.5), dict(max_hits=0), dict(max_hits=5000), dict(blank_index=99)):
        with pytest.raises(ValueError):
            kwm.KeywordSpotter(LABELS, ["A"], **bad)
    with pytest.raises(ValueError, match="kind"):
        sp.spot(None, None, kind="nope")


def test_header_and_binding_name_the_same_entry_points():
    from deepspeech.pytorch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ds2hip.h")).read()
    declared = set(re.findall(r"\b(ds2_kws_[a-z0-9_]+)\s*\(", hdr))
    bound = {n for n in _lib.SIGNATURES if n.startswith("ds2_kws_")}
    assert declared == bound
    assert {"ds2_kws_state_bytes", "ds2_kws_ws_bytes", "ds2_kws_reset", "ds2_kws_feed"} <= declared
    feed = re.search(r"int ds2_kws_feed\(([^;]*)\);", hdr).group(1)
    assert len(feed.split(",")) == len(_lib.SIGNATURES["ds2_kws_feed"][1])


def test_size_queries():
    from deepspeech.pytorch_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    # [N][W][4][64] lattice words, [N][K][8] keyword words, [N][W] frame counters
    assert lib.ds2_kws_state_bytes(100, 126, 1000) == (100 * 126 * 256 + 100 * 1000 * 8 + 100 * 126) * 4
    assert lib.ds2_kws_out_stride(1000, 8) == 4 + 1000 * 8 * 4
    assert lib.ds2_kws_ws_bytes(3, 5, 7, 2) == (16 + 3 * 7 + 3 * 7 * 2 * 3) * 4
    assert lib.ds2_kws_ws_bytes(1, 0, 1, 4097) == -1 and lib.ds2_kws_state_bytes(0, 1, 1) == -1
