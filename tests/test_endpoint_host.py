"""Host checks of endpointing: the rule's two restatements against each other, the sub-feed splitter, the
planted inputs' edges, the refusals and the ABI's declarations.  No GPU."""
import os
import re

import numpy as np
import pytest

import endpoint_reference as R

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NAMES = ["ds2_endpoint_state_bytes", "ds2_endpoint_ring_bytes", "ds2_endpoint_reset", "ds2_endpoint_feed", "ds2_endpoint_close",
         "ds2_endpoint_gather", "ds2_endpoint_commit"]


def _random_masks(rng, count):
    for _ in range(count):
        T = int(rng.integers(0, 120))
        kind = rng.integers(0, 3)
        if kind == 0:
            yield rng.random(T) < rng.random()
        else:                                    # runs, as speech has them
            out = []
            while len(out) < T:
                out += [bool(rng.integers(0, 2))] * int(rng.integers(1, 9 if kind == 1 else 30))
            yield np.array(out[:T], bool)


def test_the_walk_equals_the_enumeration_of_candidate_ends():
    rng = np.random.default_rng(1)
    reasons = set()
    for silent in _random_masks(rng, 600):
        mt, ml, ms = int(rng.integers(1, 8)), int(rng.integers(1, 12)), int(rng.integers(1, 25))
        for final in (False, True):
            a = R.segments_walk(silent, mt, ml, ms, final)
            assert a == R.segments_enumerate(silent, mt, ml, ms, final), (silent.astype(int).tolist(), mt, ml, ms)
        reasons |= {r for _, _, r in a}
        # the segments tile the stream, and none is longer than max_segment
        assert [s for s, _, _ in a] == [0] + [e + 1 for _, e, _ in a[:-1]] and a[-1][1] == len(silent) - 1
        assert all(e - s + 1 <= ms for s, e, _ in a)
    assert reasons == {"silence", "leading", "length", "final"}


def test_nan_and_the_threshold_itself_are_not_silent():
    thr = np.float32(0.8)
    got = R.silent_mask([np.nan, thr, np.nextafter(thr, np.float32(1)), np.nextafter(thr, np.float32(0)), 1.0, 0.0], 0.8)
    assert got.tolist() == [False, False, True, False, True, False]


def test_every_split_gives_the_unsplit_rule_and_no_sub_feed_holds_two_endpoints():
    from deepspeech.pytorch_amd.decoder import Endpointer, split_feed
    rng = np.random.default_rng(2)
    most = 0
    for silent in _random_masks(rng, 300):
        mt, ml, ms = int(rng.integers(1, 8)), int(rng.integers(1, 12)), int(rng.integers(1, 25))
        limit = Endpointer(0.5, mt, ml, ms).sub_feed
        assert limit == min(mt, ml, ms)
        want = R.segments_walk(silent, mt, ml, ms, final=False)
        w, got, t = R.Walker(mt, ml, ms), [], 0
        while t < len(silent):
            size = int(rng.integers(0, 40))
            chunk = silent[t:t + size]
            subs = split_feed([len(chunk)], limit)
            assert [s[0] for _, _, s in subs] == R.sub_feeds(len(chunk), limit) and all(t1 - t0 == s[0] for t0, t1, s in subs)
            for t0, t1, _ in subs:
                # what the Python layer does with one device feed: the part up to the cut, then the rest, which holds no endpoint
                cut, rest, ev = w.feed(chunk[t0:t1])
                events = [ev] if ev else []
                if rest:
                    cut2, rest2, ev2 = w.feed(chunk[t0 + cut:t1])
                    assert (cut2, rest2, ev2) == (rest, 0, None), "two endpoints in one sub-feed"
                got += [(e[1], e[2], e[0]) for e in events]
                most = max(most, len(events))
            t += len(chunk)
        assert got == want and w.consumed == len(silent)
    assert most == 1


def test_split_feed_of_several_streams():
    from deepspeech.pytorch_amd.decoder import split_feed
    assert split_feed([7, 0, 3], 3) == [(0, 3, [3, 0, 3]), (3, 6, [3, 0, 0]), (6, 7, [1, 0, 0])]
    assert split_feed([0, 0], 4) == [] and split_feed([], 4) == [] and split_feed([2], 5) == [(0, 2, [2])]
    with pytest.raises(ValueError, match="limit"):
        split_feed([3], 0)


def test_the_planted_schedules_hold_every_edge():
    mt, ml, ms = R.MIN_TRAILING, R.MAX_LEADING, R.MAX_SEGMENT
    p = R.planted_probs(29, 3)
    sil = [R.silent_mask(p[n, :T, 0], R.THRESHOLD) for n, T in enumerate(R.TOTALS)]
    assert all((a == b).all() for a, b in zip(sil, R.planted_silent()))           # the probabilities follow the letters
    assert np.isnan(p[1, R.TOTALS[1]:]).all()
    segs = [R.segments_walk(s, mt, ml, ms) for s in sil]
    assert segs[0] == [(0, 4, "leading"), (5, 13, "silence"), (14, 25, "length"), (26, 37, "length"), (38, 49, "silence"),
                       (50, 56, "silence"), (57, 65, "silence"), (66, 69, "final")]
    assert segs[1][:3] == [(0, 5, "silence"), (6, 14, "silence"), (15, 19, "leading")]
    assert all(len(s) >= 6 for s in segs)                                         # five to six times max_frames and more
    sched = R.SCHEDULES[0]
    assert sched[5:14] == "SSbbSSbbb"                   # a run of min_trailing - 1 is no cut, one of min_trailing cuts at its end
    assert "b" not in sched[14:47]                      # 33 frames of speech: the two length cuts
    assert 49 - 38 + 1 == ms and sched[47:50] == "bbb"  # "silence" and "length" due on one frame: silence wins
    thr = np.float32(R.THRESHOLD)
    assert (p[0, 51:54, 0] == thr).all() and (p[0, 54:57, 0] == np.nextafter(thr, np.float32(1))).all()
    assert sched[57:61] == "bbbb" and sched[61] == "S" and ml - 1 == 4


def test_refusals():
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder, Endpointer
    from deepspeech.pytorch_amd.configs import LABELS
    e = Endpointer()
    assert (e.blank_threshold, e.min_trailing, e.max_leading, e.max_segment, e.sub_feed) == (0.8, 50, 250, 1000, 50)
    for kw, msg in ((dict(blank_threshold=0.0), "blank_threshold"), (dict(blank_threshold=1.0), "blank_threshold"),
                    (dict(blank_threshold=float("nan")), "blank_threshold"), (dict(min_trailing=0), "min_trailing"),
                    (dict(max_leading=0), "max_leading"), (dict(max_segment=-3), "max_segment"), (dict(min_trailing=2.5), "min_trailing")):
        with pytest.raises(ValueError, match=msg):
            Endpointer(**kw)
    # a segment must fit the node pool; refused before any device memory is touched
    with pytest.raises(ValueError, match="max_segment=1000 passes the stream's max_frames=999"):
        BeamCTCDecoder(LABELS, beam_width=4).stream(2, 999, endpoint=e)


def test_entries_are_declared_bound_and_exported():
    from deepspeech.pytorch_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ds2hip.h")).read()
    assert "ds2_endpoint.hip" in build.SOURCES
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"^(?:int|long) %s\(([^;]*)\);" % name, hdr, re.M)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    # the size queries are host-only
    assert lib.ds2_endpoint_state_bytes(3) == 3 * 32 and lib.ds2_endpoint_state_bytes(0) == 0
    R_, S = 100, 1000
    assert lib.ds2_endpoint_ring_bytes(2, 8, R_, S) == 2 * 8 * (4 + 3 * R_ + 2 * R_ * S) * 4
    assert lib.ds2_endpoint_ring_bytes(2, 0, 1, 5) == 0 and lib.ds2_endpoint_ring_bytes(2, 8, 1, 0) == 0
    # refusals before any launch: null pointers and bad counts are DS2_ERR_ARG as for the beam stream's entries
    assert lib.ds2_endpoint_reset(None, 3, None, None) == 1002 and lib.ds2_endpoint_close(None, 3, None, None, None) == 1002
    assert lib.ds2_endpoint_feed(None, 0, 0, 3, 4, 29, None, 0, 0.8, 3, 5, 12, None, None, None, None, None) == 1002
    assert lib.ds2_endpoint_gather(None, 0, 0, 3, 4, 29, None, None, None, None) == 1002
    assert lib.ds2_endpoint_commit(None, None, None, 12, 1, None, None, None, 3, None, None, 8, None) == 1002
