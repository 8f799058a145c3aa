"""GPU checks of the stream pool: ds2_stream_conv1_rows / _conv2_rows / _lookahead_rows and
streaming.StreamPool.

Kernel level: the row-table kernels against the fp64 window functions of stream_exact_reference.py, row by row (fixtures.relerr
<= fixtures.TOL[dtype]): 3 rows on a pool of 5 slots, slots [4, 0, 2], permuted source rows, both buffers of every slot filled
with 7.0 so that a fresh row must read its carry as zero; per-row offsets and counts that cross the tiles; the next carry against
the window's tail, exactly; the buffer that was read, and both buffers of every slot that is not in the feed, bit for bit.
Model level: test_stream_pool_host.SCHEDULE (streams that join, pause, end and re-use a slot) per stream against the fp64 oracle
of that utterance alone (fp32: 1e-4, the bound of test_gpu_stream_exact.py; bf16: no worse than twice the one-shot bf16
forward's own error), the transcripts after every feed, two golden fixtures, and a pool in lock step against
StreamingTranscriber(carry_context=True), bit for bit."""
import numpy as np
import pytest
import torch

from fixtures import DEV, TOL, Fixture, cu, np64, relerr, rnd
from oracle import ds2_oracle as O
from stream_exact_reference import K, conv_window, lookahead_window, window
from test_gpu_model import build
from test_gpu_stream_exact import SYNTH_CHUNKS, _bn, _synth_case
from test_stream_pool_host import AUDIO, LENGTHS, SCHEDULE, oracle_probs, synth_inputs, utterance

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
S = 5                                                   # slots of the kernel-level pools


class _Slots:
    """what a session keeps per slot for ONE stage: which buffer holds the carry, whether it still reads as zero, and the fp64
    reference carry"""

    def __init__(self, bit, zero):
        self.bit, self.cur, self.fresh, self.ref = bit, [0] * S, [True] * S, [zero.copy() for _ in range(S)]

    def words(self, slot):
        return self.bit * self.cur[slot], self.bit * int(self.fresh[slot])

    def advance(self, slot, nxt):
        self.cur[slot] ^= 1
        self.fresh[slot], self.ref[slot] = False, nxt


def _check_carries(st, carry, before, slots, view, want):
    """carry / before: the two buffers after / before the launch; view(buffer, slot) the slot's part; want[slot] the next carry"""
    for s in range(S):
        if s in slots:
            c = st.cur[s]
            assert torch.equal(view(carry[c], s), view(before[c], s)), s                     # the buffer that was read
            assert torch.equal(view(carry[1 - c], s), want[s]), s                            # next carry = the window's tail, exactly
        else:
            for b in (0, 1):
                assert torch.equal(view(carry[b], s), view(before[b], s)), s                 # an absent slot keeps both buffers


# ---- conv1 --------------------------------------------------------------------------------------------------------------------
# per feed: Tc and the rows (slot, source row, len, off1, cnt1) in table order.  Counts (65, 64, 0) around the 64-frame tile with
# offsets 0 / 1 / 5; then a chunk shorter than the carry; then two rows only, one of them with nothing new (a plain copy)
CONV1_FEEDS = [(133, [(4, 2, 133, 0, 65), (0, 0, 131, 1, 64), (2, 1, 3, 5, 0)]),
               (130, [(4, 1, 3, 1, 2), (0, 2, 1, 1, 1), (2, 0, 130, 0, 63)]),
               (5, [(2, 1, 5, 5, 1), (4, 0, 0, 0, 0)])]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F0", [161, 81])
def test_conv1_rows_chain_of_feeds(F0, dtype):
    from deepspeech.pytorch_amd import ops
    rng = np.random.default_rng(F0)
    w = rng.normal(0, 1 / np.sqrt(451), (32, 1, 41, 11)).astype(np.float32).astype(np.float64)
    b = rng.normal(0, 0.1, 32).astype(np.float32).astype(np.float64)
    _, scale, shift = _bn(rng)
    w1k, b1 = cu(w.reshape(32, 451).T), cu(b)
    carry = [torch.full((S, F0, K), 7.0, device=DEV) for _ in range(2)]
    st = _Slots(1, np.zeros((1, 1, F0, K)))
    for Tc, rows in CONV1_FEEDS:
        x = rng.standard_normal((len(rows), 1, F0, Tc)).astype(np.float32)
        J = max(r[4] for r in rows)
        table = [(slot, src) + st.words(slot) + (ln, off, cnt, 0, 0, 0, 0) for slot, src, ln, off, cnt in rows]
        before = [c.clone() for c in carry]
        y = ops.stream_conv1_rows(cu(x), carry, ops.stream_rows(table, S, len(rows), Tc, DEV)[0], w1k, b1, scale, shift, J, dtype)
        assert y.shape[0] == len(rows) and y.shape[2] == J
        want_carry = {}
        for r, (slot, src, ln, off, cnt) in enumerate(rows):
            v, nxt = window(st.ref[slot], x[src:src + 1].astype(np.float64), [ln], 3)
            want = conv_window(v, off, J, w, b, np64(scale), np64(shift), np.zeros(32), np.full(32, 1.0 - O.BN_EPS), 2, [cnt])
            got = np64(y[r:r + 1]).transpose(0, 3, 1, 2)                        # [1][F1][J][32] -> (1, 32, F1, J), table order
            assert got.shape == want.shape
            if cnt:
                e = relerr(got, want)
                print("conv1 rows F0=%d %s feed Tc=%d row %s: relerr %.2e" % (F0, dtype, Tc, (slot, src, ln, off, cnt), e))
                assert e <= TOL[dtype]
            assert not got[:, :, :, cnt:].any()                                 # frames j >= cnt are zeros
            want_carry[slot] = cu(nxt[0, 0])
        _check_carries(st, carry, before, want_carry, lambda buf, s: buf[s], want_carry)
        for slot in want_carry:
            st.advance(slot, np64(want_carry[slot])[None, None])


# ---- conv2 --------------------------------------------------------------------------------------------------------------------
# per feed: Jin and the rows (slot, cnt1, off2, cnt2) in table order (cnt2 descending).  Counts (33, 32, 0) around the
# 32-position tile with n_rnn = 2: X0 has row stride 2 and the third row only moves its carry; then that row emits after its
# carry-only feed, and a row brings fewer activations than the carry holds; then two rows; then a launch without any output
CONV2_FEEDS = [(38, [(4, 38, 0, 33), (0, 37, 1, 32), (2, 3, 5, 0)]),
               (31, [(2, 31, 0, 31), (4, 6, 0, 3), (0, 3, 1, 2)]),
               (2, [(0, 2, 3, 1), (4, 0, 0, 0)]),
               (1, [(2, 1, 0, 0)])]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F0", [161, 81])
def test_conv2_rows_chain_of_feeds(F0, dtype):
    from deepspeech.pytorch_amd import ops
    rng = np.random.default_rng(F0 + 1)
    F1, F2 = ops.conv_rows(F0)
    rin, rld = 32 * F2, (32 * F2 + 63) // 64 * 64
    assert rld > rin                                                            # both geometries have pad columns
    w = rnd(rng.normal(0, 1 / np.sqrt(32 * 21 * 11), (32, 32, 21, 11)), dtype)
    b = rng.normal(0, 0.1, 32).astype(np.float32).astype(np.float64)
    _, scale, shift = _bn(rng)
    w2t, b2 = cu(w.transpose(2, 3, 0, 1), dtype), cu(b)
    carry = [torch.full((S, F1, K, 32), 7.0, device=DEV, dtype=dtype) for _ in range(2)]
    st = _Slots(2, np.zeros((1, 32, F1, K)))
    for Jin, rows in CONV2_FEEDS:
        a1 = rnd(rng.uniform(0, 4, (len(rows), 32, F1, Jin)), dtype)            # post-Hardtanh activations as stored
        J = max(r[3] for r in rows)
        n_rnn = sum(r[3] > 0 for r in rows)
        table = [(slot, r) + st.words(slot) + (0, 0, cnt1, off, cnt2, 0, 0) for r, (slot, cnt1, off, cnt2) in enumerate(rows)]
        before = [c.clone() for c in carry]
        guard = torch.full((J * n_rnn + 2, rld), 7.0, device=DEV, dtype=dtype)
        x0 = guard[:J * n_rnn]
        ops.stream_conv2_rows(cu(a1.transpose(0, 2, 3, 1), dtype), carry, ops.stream_rows(table, S, len(rows), 0, DEV)[0], n_rnn, w2t, b2,
                              scale, shift, J, rld, F0=F0, out=x0)
        assert (guard[J * n_rnn:] == 7.0).all()                                 # rows without an RNN frame write no X0 row
        got = np64(x0).reshape(J, n_rnn, rld)
        assert not got[:, :, rin:].any()                                        # the zero pad columns of the sequence layout
        want_carry = {}
        for r, (slot, cnt1, off, cnt2) in enumerate(rows):
            v, nxt = window(st.ref[slot], a1[r:r + 1], [cnt1], 3)
            want_carry[slot] = cu(nxt[0].transpose(1, 2, 0), dtype)
            if r >= n_rnn:
                continue
            want = conv_window(v, off, J, w, b, np64(scale), np64(shift), np.zeros(32), np.full(32, 1.0 - O.BN_EPS), 1, [cnt2])
            feat = got[:, r, :rin].reshape(J, 1, F2, 32).transpose(1, 3, 2, 0)  # feature f*32 + c -> (1, 32, F2, J)
            e = relerr(feat, want)
            print("conv2 rows F0=%d %s feed Jin=%d row %s: relerr %.2e" % (F0, dtype, Jin, (slot, cnt1, off, cnt2), e))
            assert e <= TOL[dtype]
            assert not feat[:, :, :, cnt2:].any()
        _check_carries(st, carry, before, want_carry, lambda buf, s: buf[s], want_carry)
        for slot in want_carry:
            st.advance(slot, np64(want_carry[slot]).transpose(2, 0, 1)[None])


# ---- lookahead ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [16, "padded 50"])
@pytest.mark.parametrize("ctx", [1, 3, 20])
def test_lookahead_rows_chain_of_feeds(ctx, H, dtype):
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd.model import _padded_hidden
    Ht = 50 if H == "padded 50" else H
    H = _padded_hidden(50, "gru", 32, False) if H == "padded 50" else H
    assert H >= Ht and H % 16 == 0
    rng, Kl = np.random.default_rng(ctx + H), ctx - 1
    w = np.zeros((H, 1, ctx))
    w[:Ht] = rng.normal(0, 1 / np.sqrt(ctx), (Ht, 1, ctx)).astype(np.float32)
    wd = cu(w[:, 0])
    carry = [torch.full((Kl, S, H), 7.0, device=DEV, dtype=dtype) for _ in range(2)] if Kl else [None, None]
    st = _Slots(4, np.zeros((Kl, 1, H)))
    # per feed: Jin and the rows (slot, cnt2, off3, cnt3) in table order: the start of a stream (nothing carried, reads beyond the
    # chunk) with counts (17, 16, 5) around the one-shot kernel's 16-frame block; short feeds, one without an output; two rows
    feeds = [(20, [(4, 20, Kl, 17), (0, 18, 0, 16), (2, 6, min(1, Kl), 5)]),
             (5, [(0, 5, 0, 3), (2, 2, 0, 2), (4, 1, 0, 0)]),
             (4, [(2, 4, 0, 4), (4, 1, min(2, Kl), 1)])]
    for Jin, rows in feeds:
        n = len(rows)
        x = rnd(rng.uniform(-1, 1, (Jin, n, H)) * (np.arange(H) < Ht), dtype)
        J = max(r[3] for r in rows)
        table = [(slot, r) + st.words(slot) + (0, 0, 0, 0, cnt2, off, cnt3) for r, (slot, cnt2, off, cnt3) in enumerate(rows)]
        before = [c.clone() for c in carry] if Kl else None
        y = ops.stream_lookahead_rows(cu(x.reshape(Jin * n, H), dtype), carry, ops.stream_rows(table, S, n, 0, DEV)[0], wd, n, S, H, J)
        got = np64(y).reshape(J, n, H)
        want_carry = {}
        for r, (slot, cnt2, off, cnt3) in enumerate(rows):
            v, nxt = window(st.ref[slot], x[:, r:r + 1], [cnt2], 0)
            want = lookahead_window(v, off, J, w)[:, 0]
            want[cnt3:] = 0                                                     # rows t >= cnt3 are zeros
            e = relerr(got[:, r], want)
            print("lookahead rows ctx=%d H=%d %s feed Jin=%d row %s: relerr %.2e" % (ctx, H, dtype, Jin, (slot, cnt2, off, cnt3), e))
            assert e <= TOL[dtype]
            assert not got[cnt3:, r].any() and not got[:, r, Ht:].any()         # ... and the padded units stay exactly 0
            want_carry[slot] = cu(nxt[:, 0], dtype)
        if Kl:
            _check_carries(st, carry, before, want_carry, lambda buf, s: buf[:, s], want_carry)
        for slot in want_carry:
            st.advance(slot, np64(want_carry[slot])[:, None])


# ---- model level: the schedule --------------------------------------------------------------------------------------------------
def _decoder(fx, kind):
    from deepspeech.pytorch_amd import decoder as D
    return D.GreedyDecoder(fx.labels) if kind == "greedy" else D.BeamCTCDecoder(fx.labels, beam_width=8)


def _decode_alone(dec, frames):
    """decoder.decode on one stream's own emitted frames: (strings, offsets) of its single entry, ('' for no frame)"""
    if not frames:
        return None
    p = torch.cat(frames)[None]
    strings, offsets = dec.decode(p, torch.tensor([p.shape[1]], dtype=torch.int))
    return strings[0], offsets[0]


def _run_schedule(m, dec, inputs, check_text=True, **kw):
    """Runs SCHEDULE on a pool of 4 slots.  Returns (per stream the emitted frames as a list of (cnt3, C) tensors, the slots the
    streams had, the pool); asserts on the way what every feed must keep."""
    from deepspeech.pytorch_amd.streaming import StreamPool, plan_feed
    pool = StreamPool(m, dec, 4, **kw)
    ctx, F0 = int(m.lookahead[0].context), inputs.shape[2]
    slot, had, fed, got = {}, {}, {}, {n: [] for n in LENGTHS}
    for i, step in enumerate(SCHEDULE):
        for n in step.get("close", ()):
            pool.close(slot.pop(n))
        for n in step.get("open", ()):
            slot[n] = had[n] = pool.open()
            fed[n] = 0
            assert pool.frames(slot[n]) == 0 and slot[n] not in pool.last_output and pool.finish(slot[n])[0] == ['']
        absent = {n: (pool.last_output.get(s), pool.finish(s)) for n, s in slot.items()}
        if "end" in step:
            names, lens, final = list(step["end"]), [0] * len(step["end"]), list(step["end"])
            texts = pool.end([slot[n] for n in names])
        else:
            names, final = [n for n, _ in step["feed"]], list(step.get("final", ()))
            lens = [LENGTHS[n] - fed[n] if c == "rest" else c for n, c in step["feed"]]
            x = torch.full((len(names), 1, F0, max(lens)), 3.0, device=DEV)    # whatever lies beyond a row's length is not read
            for r, n in enumerate(names):
                x[r, :, :, :lens[r]] = inputs[AUDIO[n], :, :, fed[n]:fed[n] + lens[r]]
            texts = pool.feed([slot[n] for n in names], x, lens, final=[slot[n] for n in final])
        assert len(texts) == len(names)
        for r, n in enumerate(names):
            p = plan_feed(fed[n], lens[r], ctx, n in final)                     # the stream's OWN plan
            out = pool.last_output.get(slot[n])
            assert (0 if out is None else out.shape[0]) == p.j3_new - p.j3_old, (i, n)
            if out is not None:
                got[n].append(out.clone())
            fed[n] += lens[r]
            assert pool.frames(slot[n]) == sum(g.shape[0] for g in got[n]) == p.j3_new
            if check_text:
                alone = _decode_alone(dec, got[n])
                assert texts[r] == ('' if alone is None else alone[0][0]), (i, n)           # the transcript after every feed
        for n, s in slot.items():
            if n not in names:                                                  # a stream that is not in the feed keeps everything
                out, (strings, offsets) = absent[n]
                assert pool.last_output.get(s) is out
                now = pool.finish(s)
                assert now[0] == strings and all(torch.equal(u, v) for u, v in zip(now[1], offsets)), (i, n)
        if i == 0:
            assert pool.latency_frames == 54 and got["a"][0].shape[0] == 1      # exactly the latency: one frame
        if i == 2:
            assert "a" in slot and "a" not in names                             # feed 3 is the one a sits out
    return got, had, slot, pool


@pytest.fixture(scope="module")
def synth_dev():
    return torch.from_numpy(synth_inputs()).to(DEV)


@pytest.mark.parametrize("kind", ["greedy", "beam"])
def test_fp32_schedule_matches_the_oracle_per_stream_and_decodes_like_decode(kind, synth_dev):
    fx = Fixture("gru_uni_la")
    m = build(fx, 32).eval()
    dec = _decoder(fx, kind)
    got, had, slot, pool = _run_schedule(m, dec, synth_dev, max_frames=80)
    assert had["d"] == had["a"] and len({had[n] for n in "abc"}) == 3           # d took the slot that a left
    for n in LENGTHS:                                                           # d as well: its slot was fresh
        want = oracle_probs(n)
        p = np64(torch.cat(got[n]))
        assert p.shape == want.shape, n
        err = np.abs(p - want).max()
        print("pool %s stream %s (%d frames): vs oracle %.2e" % (kind, n, LENGTHS[n], err))
        assert err <= 1e-4
    for n in "bcd":                                                             # the slots still open
        strings, offsets = _decode_alone(dec, got[n])
        fin = pool.finish(slot[n])
        assert fin[0] == strings and len(fin[1]) == len(offsets) and all(torch.equal(u, v) for u, v in zip(fin[1], offsets)), n
    assert any(pool.finish(slot[n])[0][0] for n in "bcd")
    with pytest.raises(ValueError, match="ended"):
        pool.feed([slot["b"]], synth_dev[:1, :, :, :5].contiguous(), [5])


def test_bf16_schedule_is_no_worse_than_twice_the_one_shot_bf16_forward(synth_dev):
    """test_gpu_stream_exact.py's rule and margin, per stream: e_oneshot is the model's own one-shot bf16 forward of that utterance"""
    fx = Fixture("gru_uni_la")
    m = build(fx, "bf16").eval()
    got, _, _, _ = _run_schedule(m, _decoder(fx, "greedy"), synth_dev, check_text=False)
    for n in LENGTHS:
        want = oracle_probs(n)
        x = torch.from_numpy(utterance(synth_inputs(), n)).to(DEV)
        with torch.no_grad():
            one = np64(m(x, torch.tensor([LENGTHS[n]], dtype=torch.int))[0])[0, :want.shape[0]]
        e_oneshot, e_stream = np.abs(one - want).max(), np.abs(np64(torch.cat(got[n])) - want).max()
        print("pool bf16 stream %s: e_stream %.3e, e_oneshot %.3e" % (n, e_stream, e_oneshot))
        assert e_stream <= 2 * e_oneshot


# ---- model level: golden fixtures with staggered starts and early ends ----------------------------------------------------------
def _run_staggered(m, dec, x, lengths, starts, chunks):
    """Stream k opens at tick starts[k] and is fed its next chunk (chunks cycled, the last one final) at every tick until it ends.
    Returns the emitted probabilities per stream, (frames, C) fp64."""
    from deepspeech.pytorch_amd.streaming import StreamPool, plan_feed
    N, ctx = len(lengths), int(m.lookahead[0].context)
    pool = StreamPool(m, dec, N)
    slot, fed, nfeeds, done, got = {}, [0] * N, [0] * N, [False] * N, [[] for _ in range(N)]
    tick = 0
    while not all(done):
        for k in range(N):
            if starts[k] == tick:
                slot[k] = pool.open()
        rows = [k for k in range(N) if k in slot and not done[k]]
        lens = [min(chunks[nfeeds[k] % len(chunks)], lengths[k] - fed[k]) for k in rows]
        final = [k for k, c in zip(rows, lens) if fed[k] + c == lengths[k]]
        xc = torch.zeros((len(rows), 1, x.shape[2], max(lens)), device=DEV)
        for r, k in enumerate(rows):
            xc[r, :, :, :lens[r]] = x[k, :, :, fed[k]:fed[k] + lens[r]]
        pool.feed([slot[k] for k in rows], xc, lens, final=[slot[k] for k in final])
        for r, k in enumerate(rows):
            p = plan_feed(fed[k], lens[r], ctx, k in final)
            out = pool.last_output.get(slot[k])
            assert (0 if out is None else out.shape[0]) == p.j3_new - p.j3_old, (tick, k)
            if out is not None:
                got[k].append(np64(out))
            fed[k] += lens[r]
            nfeeds[k] += 1
            done[k] = k in final
        tick += 1
    return [np.concatenate(g) for g in got], tick


@pytest.mark.parametrize("name,starts,chunks", [("lstm_uni_la", (0, 0), (17, 11, 21, 9)), ("gru_uni_h50_la40_c45", (0, 1, 2, 4), (17, 11, 21))])
def test_fp32_golden_fixture_streams_end_on_their_own(name, starts, chunks):
    from deepspeech.pytorch_amd import decoder as D
    fx = Fixture(name)
    x = torch.from_numpy(np.ascontiguousarray(fx.batch()[0])).to(DEV)
    lengths = [int(v) for v in fx.z["input_sizes"]]
    m = build(fx, 32).eval()
    got, ticks = _run_staggered(m, D.GreedyDecoder(fx.labels), x, lengths, starts, chunks)
    if name == "lstm_uni_la":
        assert lengths == [66, 40] and ticks == 5                               # the 40-frame clip ends in feed 3, two feeds early
    out_lens, gold = fx.z["output_lengths"], fx.z["eval_probs"].astype(np.float64)
    for n in range(len(lengths)):
        assert got[n].shape[0] == out_lens[n]
        err = np.abs(got[n] - gold[n, :out_lens[n]]).max()
        print("%s clip %d (%d frames, start %d): pool vs golden eval_probs %.2e" % (name, n, lengths[n], starts[n], err))
        assert err <= 1e-4


# ---- lock step equals the existing session, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["greedy", "beam"])
def test_pool_in_lock_step_equals_the_streaming_transcriber_bit_for_bit(kind):
    from deepspeech.pytorch_amd.streaming import StreamingTranscriber, StreamPool
    fx, x, lengths, _ = _synth_case()
    m = build(fx, 32).eval()
    chunks = list(SYNTH_CHUNKS) + [x.shape[3] - sum(SYNTH_CHUNKS)]
    ref = StreamingTranscriber(m, _decoder(fx, kind), carry_context=True, max_frames=80)
    pool = StreamPool(m, _decoder(fx, kind), 2, max_frames=80)
    slots = [pool.open(), pool.open()]
    pos, emitted = 0, 0
    for i, c in enumerate(chunks):
        last = i == len(chunks) - 1
        lens = [g - pos for g in lengths] if last else [c, c]
        xc = x[:, :, :, pos:pos + c].contiguous()
        want_text = ref.feed(xc, lens, final=last)
        text = pool.feed(slots, xc, lens, final=slots if last else ())
        assert text == want_text, i
        if ref.last_output is None:
            assert not any(s in pool.last_output for s in slots)
        else:
            probs, sizes = ref.last_output
            for n, s in enumerate(slots):
                assert pool.last_output[s].shape[0] == sizes[n]
                assert torch.equal(pool.last_output[s], probs[n, :sizes[n]]), (i, n)
            emitted += 1
        pos += c
    assert emitted >= 3 and [pool.frames(s) for s in slots] == ref.frames
    want = ref.finish()
    for n, s in enumerate(slots):
        fin = pool.finish(s)
        assert fin[0] == want[0][n] and all(torch.equal(u, v) for u, v in zip(fin[1], want[1][n]))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_pool_refusals_on_the_device():
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.streaming import StreamPool
    bi = Fixture("gru_bi_tiny")
    with pytest.raises(ValueError, match="uni-directional"):
        StreamPool(build(bi, 32), D.GreedyDecoder(bi.labels), 2)
    fx = Fixture("gru_uni_la")
    m = build(fx, 32).eval()
    x = torch.from_numpy(np.ascontiguousarray(fx.batch()[0][:2, :, :, :64])).to(DEV)
    pool = StreamPool(m, D.BeamCTCDecoder(fx.labels, beam_width=8), 2, max_frames=8)
    a, b = pool.open(), pool.open()
    with pytest.raises(ValueError, match="full"):
        pool.open()
    with pytest.raises(ValueError, match="twice"):
        pool.feed([a, a], x, [64, 64])
    with pytest.raises(ValueError, match="not an open slot"):
        pool.feed([a, 2], x, [64, 64])
    pool.feed([b, a], x, [64, 60])                                              # 6 output frames for b, 4 for a
    assert (pool.frames(a), pool.frames(b)) == (4, 6)
    with pytest.raises(ValueError, match="max_frames"):
        pool.feed([b], x[:1, :, :, :10].contiguous(), [10])                     # 5 more would pass 8; nothing is launched
    assert pool.frames(b) == 6
    with pytest.raises(ValueError, match="max_frames"):
        pool.end([a])                                                           # a's 30 output frames in all pass 8 as well
    assert pool.feed([a], x[:1, :, :, :1].contiguous(), [0]) == [pool.finish(a)[0][0]]      # a feed of nothing is no refusal
    pool.close(a)
    with pytest.raises(ValueError, match="not an open slot"):
        pool.feed([a], x[:1, :, :, :10].contiguous(), [10])                     # closed
    g = StreamPool(m, D.GreedyDecoder(fx.labels), 1)
    s = g.open()
    assert g.feed([s], x[:1], [64], final=[s]) == g.finish(s)[0] and g.frames(s) == 32
    with pytest.raises(ValueError, match="ended"):
        g.end([s])                                                              # a stream that has ended, until close() and open()
    g.close(s)
    assert g.open() == s and g.frames(s) == 0
