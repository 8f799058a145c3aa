"""Host-side checks of exact chunked inference, no GPU needed: the fp64 restatement of the chunked
algorithm (stream_exact_reference.py, stated carries only) against the oracle's one-shot eval forward, the index plan
(streaming.plan_feed == ds2_stream_plan) and its invariants, the declared signatures, and the session's argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from fixtures import Fixture
from oracle import ds2_oracle as O
from stream_exact_reference import stream_all

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ds2_stream_plan", "ds2_stream_state_bytes", "ds2_stream_conv1", "ds2_stream_conv2", "ds2_stream_lookahead"]
FIXTURES = ["gru_uni_la", "lstm_uni_la", "gru_uni_h50_la40_c45"]
# (input frames per feed, streams); the last feed is final and 3 frames shorter on stream 1
SPLITS = [((17, 11, 21, 12), 2), ((1, 2, 3, 5, 50), 2), ((60,), 1), ((59, 1), 1), ((7,) * 8 + (4,), 2), ((30, 31), 2), ((1,) * 61, 1)]
# fp64 and the same operations in both arms, sums of at most 32 * 21 * 11 = 7392 terms: rounding differences of a few 1e-16 at
# unit scale; an index error shows as O(1e-2)
BOUND = 1e-10


@pytest.fixture(scope="module")
def lib():
    from deepspeech.pytorch_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


_ONE_SHOT = {}


def one_shot(name, N, T):
    """(inputs zero beyond every stream's length, lengths, the oracle's eval probabilities, output lengths), computed once"""
    key = (name, N, T)
    if key not in _ONE_SHOT:
        fx = Fixture(name)
        x = np.ascontiguousarray(fx.batch()[0][:N, :, :, :T]).astype(np.float64)
        lengths = np.array([T, T - 3][:N])
        for n in range(N):
            x[n, :, :, lengths[n]:] = 0
        P = {k: v.astype(np.float64) for k, v in fx.params().items()}
        out, out_lens, _, _ = O.model_forward(P, fx.cfg, x, lengths, train=False, keep_cache=False)
        _ONE_SHOT[key] = (fx, P, x, lengths, out, out_lens)
    return _ONE_SHOT[key]


@pytest.mark.parametrize("chunks,N", SPLITS)
@pytest.mark.parametrize("name", FIXTURES)
def test_chunked_restatement_equals_the_one_shot_eval_forward(name, chunks, N):
    fx, P, x, lengths, out, out_lens = one_shot(name, N, sum(chunks))
    got, ref = stream_all(P, fx.cfg, x, lengths, chunks, F0=x.shape[2])
    for n in range(N):
        assert got[n].shape[0] == out_lens[n]                                   # every frame emitted, once
        err = np.abs(got[n] - out[n, :out_lens[n]]).max()
        print("%s %s stream %d: max |dp| = %.2e" % (name, chunks, n, err))
        assert err <= BOUND
    for p, c in zip(ref.plans[:-1], chunks):                                    # the stated carries were enough in every feed
        _check_reads_stay_in_the_window(p, c, fx.cfg["lookahead_context"])


def _check_reads_stay_in_the_window(p, chunk, ctx):
    J1, J2, J3 = p.j1_new - p.j1_old, p.j2_new - p.j2_old, p.j3_new - p.j3_old
    assert (p.k_in, p.k_act, p.k_la) == (10, 10, ctx - 1)
    assert min(p.off1, p.off2, p.off3, J1, J2, J3) >= 0                         # nothing in front of the carry is read
    assert J1 == 0 or p.off1 + 2 * (J1 - 1) + 10 <= p.k_in + chunk - 1          # ... and, when not final, nothing beyond the chunk
    assert J2 == 0 or p.off2 + (J2 - 1) + 10 <= p.k_act + J1 - 1
    assert J3 == 0 or p.off3 + (J3 - 1) + ctx - 1 <= p.k_la + J2 - 1


def c_plan(lib, G, Tc, ctx, final):
    out = (C.c_int * 12)()
    assert lib.ds2_stream_plan(G, Tc, ctx, int(final), out) == 0
    return tuple(out)


def test_plan_feed_equals_ds2_stream_plan_and_keeps_its_invariants(lib):
    from deepspeech.pytorch_amd.streaming import plan_feed
    seq = lambda G: int(O.seq_lens([G])[0]) if G > 0 else 0
    for ctx in (1, 2, 20, 40):
        for G in range(131):
            for Tc in range(71):
                for final in (False, True):
                    p = plan_feed(G, Tc, ctx, final)
                    assert tuple(p) == c_plan(lib, G, Tc, ctx, final), (G, Tc, ctx, final)
                    assert p.j1_old <= p.j1_new and p.j2_old <= p.j2_new and p.j3_old <= p.j3_new      # monotone
                    assert p.j3_new <= p.j2_new <= p.j1_new <= seq(G + Tc)
                    if final:
                        assert p.j1_new == p.j2_new == p.j3_new == seq(G + Tc)
                    else:
                        _check_reads_stay_in_the_window(p, Tc, ctx)
                        q = plan_feed(G + Tc, 0, ctx)                           # the next feed starts where this one stopped
                        assert (q.j1_old, q.j2_old, q.j3_old) == (p.j1_new, p.j2_new, p.j3_new)
    assert lib.ds2_stream_plan(-1, 1, 20, 0, (C.c_int * 12)()) != 0 and lib.ds2_stream_plan(0, 1, 0, 0, (C.c_int * 12)()) != 0
    assert lib.ds2_stream_plan(0, 1, 20, 0, None) != 0
    with pytest.raises(ValueError):
        plan_feed(0, 1, 0)


def test_retired_totals_over_random_splits_equal_get_seq_lens():
    from deepspeech.pytorch_amd.streaming import plan_feed
    rng = np.random.default_rng(0)
    for _ in range(300):
        ctx, G, tot = int(rng.choice([1, 2, 20, 40])), 0, [0, 0, 0]
        chunks = [int(c) for c in rng.integers(1, 40, size=rng.integers(1, 12))]
        for i, c in enumerate(chunks):
            p = plan_feed(G, c, ctx, final=(i == len(chunks) - 1))
            assert [p.j1_old, p.j2_old, p.j3_old] == tot
            tot = [p.j1_new, p.j2_new, p.j3_new]
            G += c
        assert tot == [int(O.seq_lens([G])[0])] * 3, (chunks, ctx)


def test_latency_is_the_first_input_count_with_an_output_frame():
    from deepspeech.pytorch_amd.streaming import plan_feed
    for ctx in (1, 2, 20, 40):
        first = next(G for G in range(400) if plan_feed(0, G, ctx).j3_new > 0)
        assert first == 2 * ctx + 14
    assert plan_feed(0, 54, 20).j3_new == 1 and plan_feed(0, 53, 20).j3_new == 0


def test_signatures_are_declared_exported_and_match_the_header(lib):
    from deepspeech.pytorch_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "ds2hip.h")).read()
    assert "ds2_stream.hip" in build.SOURCES
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name     # one ctypes type per declared argument
    assert _lib.SIGNATURES["ds2_stream_state_bytes"][0] is _lib.C.c_long


def test_state_bytes_are_the_double_buffered_aligned_carries(lib):
    al = lambda b: (b + 255) // 256 * 256
    for dtype, esz in ((0, 4), (1, 2)):
        for N in (1, 3, 32):
            for F0, F1 in ((161, 81), (81, 41)):
                for H in (16, 64, 800):
                    for ctx in (1, 3, 20, 40):
                        want = 2 * (al(N * F0 * 10 * 4) + al(N * F1 * 10 * 32 * esz) + al((ctx - 1) * N * H * esz))
                        assert lib.ds2_stream_state_bytes(dtype, N, F0, H, ctx) == want
    for bad in ((2, 1, 161, 16, 20), (0, 0, 161, 16, 20), (0, 1, 0, 16, 20), (0, 1, 161, 0, 20), (0, 1, 161, 16, 0)):
        assert lib.ds2_stream_state_bytes(*bad) == 0


def _cpu_model(name):
    from test_host import build_model
    return build_model(Fixture(name))


def test_session_refuses_what_cannot_be_exact():
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.streaming import StreamingTranscriber
    fx = Fixture("gru_bi_tiny")
    dec = D.GreedyDecoder(fx.labels)
    with pytest.raises(ValueError, match="uni-directional"):
        StreamingTranscriber(_cpu_model("gru_bi_tiny"), dec, carry_context=True)
    StreamingTranscriber(_cpu_model("gru_bi_tiny"), dec)                        # the default mode takes any model
    st = StreamingTranscriber(_cpu_model("gru_uni_la"), dec, carry_context=True)
    assert st.latency_frames == 54 and st.frames == [] and st.best() == []
    assert StreamingTranscriber(_cpu_model("gru_uni_la"), dec).latency_frames == 0
    with pytest.raises(ValueError, match="feed_wave"):
        st.feed_wave(torch.zeros(2, 4800), [4800, 4800])
    with pytest.raises(ValueError, match="not final"):
        st.feed(torch.zeros(2, 1, 161, 17), [17, 15])                           # ragged lengths belong to the final feed
    with pytest.raises(ValueError, match="descend"):
        st.feed(torch.zeros(2, 1, 161, 17), [15, 17], final=True)
    with pytest.raises(ValueError, match="spectrogram chunk"):
        st.feed(torch.zeros(2, 1, 81, 17), [17, 17])
    with pytest.raises(ValueError, match="nothing has been fed"):
        st.end()
    with pytest.raises(ValueError):
        StreamingTranscriber(_cpu_model("gru_uni_la"), dec).end()               # no end() without carry_context
