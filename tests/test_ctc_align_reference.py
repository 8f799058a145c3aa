"""CPU checks of forced alignment: the fp64 restatement (tests/ctc_align_reference.py) against enumeration of every path and
against the CTC log-likelihood of the oracle, and the host parts of deepspeech.pytorch_amd.align (string mapping, word grouping,
seconds)."""
import numpy as np
import pytest

import ctc_align_reference as R
from oracle import ds2_oracle as O

BLANK = 0


def _paths(T, ext):
    """every valid state path of T frames through the extended sequence"""
    S = len(ext)

    def grow(path):
        if len(path) == T:
            if path[-1] >= S - 2:
                yield tuple(path)
            return
        s = path[-1]
        for d in (0, 1, 2):
            b = s + d
            if b < S and (d < 2 or (b & 1 and ext[b] != ext[s])):
                yield from grow(path + [b])
    for s0 in (0, 1):
        if s0 < S:
            yield from grow([s0])


def _brute(lp, target):
    """Best path by enumeration.  The tie rule (predecessor s before s-1 before s-2, the final blank before the final label) picks,
    among the best paths, the one whose state sequence read from the last frame backwards is lexicographically largest."""
    ext = R.extended(target, BLANK)
    best = None
    for p in _paths(lp.shape[0], ext):
        key = (sum(lp[t, ext[s]] for t, s in enumerate(p)), tuple(reversed(p)))
        if best is None or key > best:
            best = key
    return (-np.inf, None) if best is None or best[0] == -np.inf else (best[0], list(reversed(best[1])))


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("L", [0, 1, 2, 3])
def test_restatement_equals_enumeration_of_all_paths(T, L):
    """3 classes + blank, log-probabilities from {0, -1/2, -1, -3/2, -inf}: sums are exact, so equal scores ARE ties and the exact
    path under the tie rule is pinned, not only the score."""
    rs = np.random.RandomState(100 * T + L)
    values = np.array([0.0, -0.5, -1.0, -1.5, -np.inf])
    ties = 0
    for trial in range(40):
        lp = values[rs.randint(0, 4 if trial % 4 else 5, size=(T, 4))]
        target = rs.randint(1, 4, size=L)
        if L >= 2 and trial % 3 == 0:
            target[1] = target[0]                                    # adjacent equal labels: no s-2 step between them
        score, path = _brute(lp, target)
        got = R.align(lp, target, BLANK)
        assert got.score == score
        if path is None:
            assert np.all(got.frame_state == -1) and np.all(got.tok_start == -1) and np.all(got.tok_end == -1) and np.all(got.tok_logp == 0)
            continue
        assert got.frame_state.tolist() == path
        assert R.collapses_to(got.frame_state, target, BLANK) and R.rescore(lp, got.frame_state, target, BLANK) == score
        ext = R.extended(target, BLANK)
        ties += sum(1 for p in _paths(T, ext) if sum(lp[t, ext[s]] for t, s in enumerate(p)) == score) > 1
        for i in range(L):
            fr = [t for t, s in enumerate(path) if s == 2 * i + 1]
            assert (got.tok_start[i], got.tok_end[i]) == (fr[0], fr[-1]) and got.tok_logp[i] == sum(lp[t, target[i]] for t in fr)
    if L >= 1 and T > L + 1:                                         # (an empty target has one path)
        assert ties > 0                                              # the cases do exercise the tie rule


def test_infeasible_and_empty_cases():
    lp = np.full((3, 4), -1.0)
    a = R.align(lp, [1, 1], BLANK)                                   # two equal labels need the blank between them: 3 frames
    assert a.score == -3.0 and a.frame_state.tolist() == [1, 2, 3]
    assert (a.tok_start.tolist(), a.tok_end.tolist(), a.tok_logp.tolist()) == ([0, 2], [0, 2], [-1.0, -1.0])
    b = R.align(lp[:2], [1, 1], BLANK)                               # one frame short: L + repeats - 1
    assert b.score == -np.inf and b.frame_state.tolist() == [-1, -1] and b.tok_start.tolist() == [-1, -1] and b.tok_logp.tolist() == [0, 0]
    assert R.align(lp[:2], [1, 2], BLANK).frame_state.tolist() == [1, 3]     # different labels: no blank needed
    e = R.align(lp, [], BLANK)                                       # empty target: the all-blank path
    assert e.score == -3.0 and e.frame_state.tolist() == [0, 0, 0] and len(e.tok_start) == 0
    assert R.align(lp[:0], [1], BLANK).score == -np.inf              # no frames
    assert R.align(lp[:1], [1, 2], BLANK).score == -np.inf
    assert not R.collapses_to([0, 1, 1], [1, 2], BLANK) and R.collapses_to([1, 3], [1, 2], BLANK)
    assert not R.collapses_to([1, 3], [1, 1], BLANK) and R.collapses_to([1, 2, 3], [1, 1], BLANK)


@pytest.mark.parametrize("seed", range(6))
def test_best_path_never_beats_the_log_likelihood(seed):
    """The best path is one term of the sum the CTC loss takes the logarithm of: score <= -nll (oracle, float64)."""
    rs = np.random.RandomState(seed)
    N, T, C = 4, 30, 6
    lens, tlens = np.array([30, 25, 12, 7]), np.array([9, 1, 12, 0])
    lp = O.log_softmax(rs.standard_normal((T, N, C)) * 3)
    targets = rs.randint(1, C, size=int(tlens.sum()))
    targets[1] = targets[0]
    _, nll, _ = O.ctc_loss_and_grad(lp, targets, lens, tlens, blank=BLANK)
    off = 0
    for n in range(N):
        a = R.align(lp[:lens[n], n], targets[off:off + tlens[n]], BLANK)
        off += tlens[n]
        if a.score == -np.inf:
            assert nll[n] == 0                                       # zero_infinity: the loss calls the same clips infeasible
        else:
            assert a.score <= -nll[n] + 1e-9 and a.score >= -nll[n] - T * np.log(3.0) * 2


# ---- host surface of deepspeech.pytorch_amd.align -----------------------------------------------------------------------------
LABELS = ["_", "'", "A", "B", "C", "D", " "]


def _chars(text, spans, fs=None):
    from deepspeech.pytorch_amd import align as A
    return [A.make_span(ch, s, e, lp, fs) for ch, (s, e, lp) in zip(text, spans)]


def test_word_grouping_with_leading_trailing_and_double_spaces():
    from deepspeech.pytorch_amd import align as A
    text = " AB  C'D "
    spans = [(0, 0, -0.5), (2, 3, -1.0), (4, 4, -0.25), (6, 6, -2.0), (7, 9, -2.0), (11, 11, -0.125), (12, 12, -0.5), (14, 15, -1.0),
             (17, 17, -4.0)]
    words = A.group_words(_chars(text, spans))
    assert [w[:4] for w in words] == [("AB", 2, 4, -1.25), ("C'D", 11, 15, -1.625)]
    assert all(w.start_s is None and w.end_s is None for w in words)
    assert A.group_words(_chars("  ", spans[:2])) == [] and A.group_words([]) == []
    assert [w[:4] for w in A.group_words(_chars("A", [(5, 7, -1.0)]))] == [("A", 5, 7, -1.0)]


def test_seconds_conversion():
    from deepspeech.pytorch_amd import align as A
    chars = _chars("A B", [(3, 4, -1.0), (5, 5, -1.0), (6, 9, -1.0)], fs=0.02)
    assert (chars[0].start_s, chars[0].end_s) == (3 * 0.02, 5 * 0.02)
    w = A.group_words(chars, 0.02)
    assert [(x.text, x.start_s, x.end_s) for x in w] == [("A", 3 * 0.02, 5 * 0.02), ("B", 6 * 0.02, 10 * 0.02)]

    class M:
        labels, blank_index = LABELS, 0

        class spect_cfg:
            window_stride = 0.01
    al = A.ForcedAligner.from_model(M)
    assert al.frame_seconds == 0.02 and al.blank_index == 0 and al.labels is LABELS


def test_transcripts_map_through_the_labels_and_unknown_characters_raise():
    from deepspeech.pytorch_amd import align as A
    al = A.ForcedAligner(LABELS, blank_index=0)
    tg, ts = al.targets_of(["AB C", "", "D'"])
    assert tg.tolist() == [2, 3, 6, 4, 5, 1] and ts.tolist() == [4, 0, 2]
    with pytest.raises(ValueError, match="'x'"):
        al.targets_of(["AB", "AxB"])
    with pytest.raises(ValueError, match="'_'"):
        al.targets_of(["A_B"])                                       # the blank is no character of a transcript
    chars, words = al.spans([2, 6, 3], [0, 2, 3], [1, 2, 5], [-1.0, -0.5, -0.25])
    assert [c[:4] for c in chars] == [("A", 0, 1, -1.0), (" ", 2, 2, -0.5), ("B", 3, 5, -0.25)]
    assert [w[:4] for w in words] == [("A", 0, 1, -1.0), ("B", 3, 5, -0.25)]


def test_flag_lists_infeasible_clips_and_clips_below_the_bar():
    from deepspeech.pytorch_amd import align as A
    mk = lambda score, frames: A.Alignment(score, score != float("-inf"), [], [], None, frames)      # noqa: E731
    als = [mk(-10.0, 10), mk(-30.0, 10), mk(float("-inf"), 10), mk(-2.0, 1), mk(-20.0, 10)]
    assert A.ForcedAligner.flag(als, -2.0) == [1, 2]
    assert A.ForcedAligner.flag(als, -0.5) == [0, 1, 2, 3, 4] and A.ForcedAligner.flag(als, -100.0) == [2]
