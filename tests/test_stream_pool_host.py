"""Host-side checks of the stream pool, no GPU needed: the per-row plan (streaming.plan_rows) over random
join and leave schedules, the fp64 restatement of chunked inference fed each stream's own chunk sequence of the GPU schedule
(one ChunkedReference(N=1) per stream) against the oracle's one-shot eval forward, the declared signatures and the row struct,
and the refusals that need no device.  SCHEDULE is also what test_gpu_stream_pool.py runs on the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from fixtures import Fixture
from oracle import ds2_oracle as O
from stream_exact_reference import ChunkedReference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ds2_stream_conv1_rows", "ds2_stream_conv2_rows", "ds2_stream_lookahead_rows"]
BOUND = 1e-10                                           # test_stream_exact_host.py's: fp64, the same operations in both arms

# The model-level schedule: three synthetic utterances on gru_uni_la's weights and d, which re-uses a's slot with a's audio.
# c and d are ended by end(), so their utterances are what they were fed: 101 frames, and the first 54 of a's.
LENGTHS = dict(a=160, b=155, c=101, d=54)
AUDIO = dict(a=0, b=1, c=2, d=0)                        # the row of the synthetic batch that a stream reads
SCHEDULE = [
    dict(open=["a"], feed=[("a", 54)]),                                         # exactly the latency: 1 frame
    dict(open=["b"], feed=[("a", 17), ("b", 23)]),
    dict(feed=[("b", 31)]),                                                     # a is absent
    dict(open=["c"], feed=[("c", 60), ("a", 1), ("b", 2)]),                     # rows in another order, 1- and 2-frame chunks
    dict(feed=[("a", "rest"), ("b", 40), ("c", 11)], final=["a"]),
    dict(close=["a"], open=["d"], feed=[("d", 54), ("b", "rest"), ("c", 30)], final=["b"]),
    dict(end=["c", "d"]),
]


def stream_feeds(name):
    """[(schedule step, input frames, final)] of one stream: its own chunk sequence, end() being a final chunk of nothing"""
    out, fed = [], 0
    for i, step in enumerate(SCHEDULE):
        for who, c in step.get("feed", ()):
            if who == name:
                c = LENGTHS[name] - fed if c == "rest" else c
                out.append((i, c, name in step.get("final", ())))
                fed += c
        if name in step.get("end", ()):
            out.append((i, 0, True))
    assert fed == LENGTHS[name] and out[-1][2] and not any(f for _, _, f in out[:-1])
    return out


def synth_inputs():
    """(3, 1, 161, 160) float32: the three synthetic utterances, a and b as test_gpu_stream_exact._synth_case has them"""
    from deepspeech.pytorch_amd import synth
    return synth.synth_batch(np.asarray([160, 155, 120]), seed=11)[0]


def utterance(inputs, name):
    return np.ascontiguousarray(inputs[AUDIO[name]:AUDIO[name] + 1, :, :, :LENGTHS[name]])


_ORACLE = {}


def oracle_probs(name):
    """the fp64 oracle's eval probabilities (Tp, C) of one utterance alone, computed once"""
    if name not in _ORACLE:
        fx = Fixture("gru_uni_la")
        P = {k: v.astype(np.float64) for k, v in fx.params().items()}
        x = utterance(synth_inputs(), name).astype(np.float64)
        out, out_lens = O.model_forward(P, fx.cfg, x, np.asarray([LENGTHS[name]]), train=False, keep_cache=False)[:2]
        _ORACLE[name] = out[0, :int(out_lens[0])]
    return _ORACLE[name]


# ---- the per-row plan -----------------------------------------------------------------------------------------------------------
def _check_row_plan(rp, fed, lens, finals, ctx):
    from deepspeech.pytorch_amd.streaming import plan_feed
    n = len(fed)
    for r in range(n):
        p = plan_feed(fed[r], lens[r], ctx, finals[r])
        assert rp.plans[r] == p
        assert (rp.off1[r], rp.off2[r], rp.off3[r]) == (p.off1, p.off2, p.off3)
        assert (rp.cnt1[r], rp.cnt2[r], rp.cnt3[r]) == (p.j1_new - p.j1_old, p.j2_new - p.j2_old, p.j3_new - p.j3_old)
        assert rp.cnt3[r] == 0 or rp.cnt2[r] > 0
    assert (rp.J1, rp.J2, rp.J3) == tuple(max(c, default=0) for c in (rp.cnt1, rp.cnt2, rp.cnt3))
    assert sorted(rp.order) == list(range(n))
    keys = [rp.cnt2[r] for r in rp.order]
    assert keys == sorted(keys, reverse=True)                                   # by cnt2 descending ...
    for a, b in zip(rp.order, rp.order[1:]):
        assert rp.cnt2[a] > rp.cnt2[b] or a < b                                 # ... and stable
    assert rp.n_rnn == sum(c > 0 for c in rp.cnt2)
    assert all(rp.cnt2[r] > 0 for r in rp.order[:rp.n_rnn]) and not any(rp.cnt2[r] for r in rp.order[rp.n_rnn:])   # a prefix


def test_row_plans_of_random_join_and_leave_schedules_tile_every_stream_exactly_once():
    from deepspeech.pytorch_amd.streaming import plan_rows
    rng = np.random.default_rng(5)
    for trial in range(60):
        ctx = int(rng.choice([1, 2, 20, 40]))
        total = [int(v) for v in rng.integers(0, 260, size=6)]                  # utterance lengths, 0 included
        start = [int(v) for v in rng.integers(0, 8, size=6)]                    # the tick at which a stream joins
        fed, done = [0] * 6, [False] * 6
        ends = [[0, 0, 0] for _ in range(6)]                                    # where every stream's three ranges stopped
        tick = 0
        while not all(done):
            rows = [k for k in range(6) if not done[k] and tick >= start[k] and rng.random() < 0.7]
            rng.shuffle(rows)
            lens, finals = [], []
            for k in rows:
                c = int(min(rng.choice([0, 1, 2, 7, 20, 53, 90]), total[k] - fed[k]))
                lens.append(c)
                finals.append(fed[k] + c == total[k] and bool(rng.random() < 0.6))
            rp = plan_rows([fed[k] for k in rows], lens, finals, ctx)
            _check_row_plan(rp, [fed[k] for k in rows], lens, finals, ctx)
            for r, k in enumerate(rows):
                p = rp.plans[r]
                assert [p.j1_old, p.j2_old, p.j3_old] == ends[k]               # every range starts where the last one stopped
                ends[k] = [p.j1_new, p.j2_new, p.j3_new]
                fed[k] += lens[r]
                done[k] = finals[r]
            tick += 1
        for k in range(6):
            Tp = int(O.seq_lens([total[k]])[0]) if total[k] > 0 else 0
            assert ends[k] == [Tp, Tp, Tp], (trial, k, total[k])                # ... and all three end at the stream's own Tp


def test_row_plan_of_the_gpu_schedule_and_its_refusals():
    from deepspeech.pytorch_amd.streaming import plan_rows
    rp = plan_rows([0, 71, 54], [60, 1, 2], [False] * 3, 20)                    # step 4 of the schedule: (c, a, b)
    _check_row_plan(rp, [0, 71, 54], [60, 1, 2], [False] * 3, 20)
    assert rp.cnt2 == [23, 1, 1] and rp.cnt3 == [4, 1, 1] and rp.order == [0, 1, 2] and rp.n_rnn == 3
    rp = plan_rows([54, 0], [17, 23], [False, False], 20)                       # step 2: b is in its first 2 * ctx + 14 frames
    assert rp.cnt2 == [8, 4] and rp.cnt3 == [8, 0] and rp.n_rnn == 2
    rp = plan_rows([0, 54, 0], [9, 17, 0], [False, False, True], 20)            # rows without an RNN frame go behind the others
    assert rp.cnt2 == [0, 8, 0] and rp.order == [1, 0, 2] and rp.n_rnn == 1 and (rp.J1, rp.J2, rp.J3) == (8, 8, 8)
    assert plan_rows([], [], [], 20).n_rnn == 0
    with pytest.raises(ValueError):
        plan_rows([0, 1], [1], [False, False], 20)
    with pytest.raises(ValueError):
        plan_rows([0], [-1], [False], 20)


# ---- the fp64 restatement, one reference per stream -----------------------------------------------------------------------------
@pytest.mark.parametrize("extra_zero_chunks", [False, True])
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_each_stream_fed_its_own_chunks_equals_its_one_shot_eval_forward(name, extra_zero_chunks):
    from deepspeech.pytorch_amd.streaming import plan_rows
    fx = Fixture("gru_uni_la")
    P = {k: v.astype(np.float64) for k, v in fx.params().items()}
    x = utterance(synth_inputs(), name).astype(np.float64)
    ref = ChunkedReference(P, fx.cfg, 1)
    feeds = [(c, f) for _, c, f in stream_feeds(name)]
    if extra_zero_chunks:                                                       # a feed that brings a present stream nothing
        feeds = [feeds[0], (0, False)] + feeds[1:-1] + [(0, False), feeds[-1]]
    got, pos = [], 0
    for c, final in feeds:
        rp = plan_rows([pos], [c], [final], fx.cfg["lookahead_context"])
        probs, sizes = ref.feed(x[:, :, :, pos:pos + c], [c], final=final)
        assert sizes[0] == rp.cnt3[0] and ref.plans[-1] == rp.plans[0]
        got.append(probs[0, :sizes[0]])
        pos += c
    got, want = np.concatenate(got), oracle_probs(name)
    assert got.shape == want.shape
    err = np.abs(got - want).max()
    print("stream %s %s: max |dp| = %.2e" % (name, [c for c, _ in feeds], err))
    assert err <= BOUND


# ---- declarations ---------------------------------------------------------------------------------------------------------------
def test_row_entries_are_declared_exported_and_the_row_struct_has_16_words():
    from deepspeech.pytorch_amd import _lib, build, ops
    build.build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ds2hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    body = re.search(r"typedef struct ds2_stream_row \{(.*?)\} ds2_stream_row;", hdr, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [f.strip() for decl in re.findall(r"int32_t([^;]*);", fields) for f in decl.split(",")]
    assert names[:11] == ["slot", "src", "cur", "fresh", "len", "off1", "cnt1", "off2", "cnt2", "off3", "cnt3"]
    assert names[11:] == ["reserved[5]"] and ops.STREAM_ROW_WORDS == 16
    # the entries refuse a null table and equal carry buffers before any launch
    one = C.c_void_p(256)
    assert lib.ds2_stream_conv1_rows(0, one, one, C.c_void_p(512), None, one, one, one, one, one, 1, 161, 4, 1, None) != 0
    assert lib.ds2_stream_conv1_rows(0, one, one, one, one, one, one, one, one, one, 1, 161, 4, 1, None) != 0
    assert lib.ds2_stream_conv2_rows(0, one, one, C.c_void_p(512), one, one, one, one, one, one, 2, 3, 161, 4, 1, 1344, None) != 0
    assert lib.ds2_stream_conv2_rows(0, one, one, C.c_void_p(512), one, one, one, one, one, one, 2, 0, 161, 4, 1, 1344, None) != 0
    assert lib.ds2_stream_lookahead_rows(2, one, one, C.c_void_p(512), one, one, one, 1, 4, 16, 3, 1, 1, None) != 0
    assert lib.ds2_stream_lookahead_rows(0, one, one, C.c_void_p(512), one, one, one, 5, 4, 16, 3, 1, 1, None) != 0


def test_row_table_checks_what_the_kernels_cannot():
    from deepspeech.pytorch_amd import ops
    row = lambda slot, src=0, cnt2=0, cnt3=0, ln=1: (slot, src, 0, 7, ln, 0, 0, 0, cnt2, 0, cnt3)
    for bad in ([row(5)], [row(-1)], [row(1), row(1, 1)], [row(0, 2)], [row(0, ln=9)], [row(0, cnt2=1), row(1, 1, cnt2=2)],
                [row(0, cnt3=1)], [(0, 0, 8, 0, 1, 0, 0, 0, 0, 0, 0)], [(0, 0, 0, 0, 1, -1, 0, 0, 0, 0, 0)], []):
        with pytest.raises(ValueError):
            ops.stream_rows(bad, 5, 2, 8, "cpu")
    table, cnt2, slots = ops.stream_rows([row(4, 1, cnt2=3, cnt3=1), row(0, 0, cnt2=2), row(2, 0)], 5, 2, 8, "cpu")
    assert table.shape == (3, 16) and table.dtype == torch.int32 and cnt2.tolist() == [3, 2, 0]
    assert slots.dtype == torch.int64 and slots.tolist() == [4, 0, 2] and table[:, :2].tolist() == [[4, 1], [0, 0], [2, 0]]


# ---- refusals that need no device -----------------------------------------------------------------------------------------------
def _cpu_model(name):
    from test_host import build_model
    return build_model(Fixture(name))


def test_pool_refuses_before_any_launch():
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.streaming import StreamPool
    fx = Fixture("gru_uni_la")
    with pytest.raises(ValueError, match="uni-directional"):
        StreamPool(_cpu_model("gru_bi_tiny"), D.GreedyDecoder(Fixture("gru_bi_tiny").labels), 2)
    m = _cpu_model("gru_uni_la")
    pool = StreamPool(m, D.BeamCTCDecoder(fx.labels, beam_width=8), 2, max_frames=3)
    assert pool.latency_frames == 54 and pool.last_output == {}
    x = torch.zeros(1, 1, 161, 80)
    with pytest.raises(ValueError, match="not an open slot"):
        pool.feed([0], x, [80])                                                 # never opened
    a, b = pool.open(), pool.open()
    assert (a, b) == (0, 1) and pool.frames(a) == 0 and pool.finish(a)[0] == ['']
    with pytest.raises(ValueError, match="full"):
        pool.open()
    with pytest.raises(ValueError, match="not an open slot"):
        pool.feed([2], x, [80])                                                 # unknown
    with pytest.raises(ValueError, match="twice"):
        pool.feed([a, a], torch.zeros(2, 1, 161, 80), [80, 80])                 # duplicated
    with pytest.raises(ValueError, match="not in this feed"):
        pool.feed([a], x, [80], final=[b])
    with pytest.raises(ValueError, match="spectrogram chunk"):
        pool.feed([a, b], x, [80, 80])
    with pytest.raises(ValueError, match="lengths"):
        pool.feed([a], x, [81])
    with pytest.raises(ValueError, match="max_frames"):
        pool.feed([a], x, [80], final=[a])                                      # 40 output frames into a beam stream of 3
    pool.close(b)
    with pytest.raises(ValueError, match="not an open slot"):
        pool.feed([b], x, [80])                                                 # closed
    assert pool.open() == b
