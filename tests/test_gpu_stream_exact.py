"""GPU checks of exact chunked inference (csrc/ds2_stream.hip, StreamingTranscriber(carry_context=True)).

Kernel level: ds2_stream_conv1 / _conv2 / _lookahead against the fp64 window functions of stream_exact_reference.py
(fixtures.relerr <= fixtures.TOL[dtype]) over chains of feeds that cross the tile edges (64 frames for conv1, 32 for conv2, the
start-of-stream offsets, chunks shorter than the carry, ragged ends), and the next carry against the window's tail, exactly.
Model level: the streamed probabilities against the real reference's golden eval_probs (fp32, 1e-4, the bound test_gpu_model.py
holds the one-shot forward to) and against the fp64 oracle (bf16: no worse than twice the one-shot bf16 forward's own error).
Session: transcripts after every feed, reset, the untouched default mode, the refusals.

lstm_uni_la's second clip has 40 input frames, fewer than the 49 the chunks (17, 11, 21) deliver before the final feed, and
streams end in the same feed: that batch is streamed as (17, 11, rest), and its first clip alone as (17, 11, 21, rest)."""
import numpy as np
import pytest
import torch

from fixtures import DEV, TOL, Fixture, cu, np64, relerr, rnd
from oracle import ds2_oracle as O
from stream_exact_reference import K, conv_window, lookahead_window, window
from test_gpu_model import build

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
CHUNKS = (17, 11, 21)                                   # then the rest, final and ragged


def _bn(rng):
    """eval BatchNorm2d of 32 channels: (gamma, beta, running_mean, running_var) and the folded (scale, shift) the kernels take"""
    g, b, rm, rv = rng.uniform(0.5, 1.5, 32), rng.normal(0, 0.3, 32), rng.normal(0, 0.2, 32), rng.uniform(0.5, 1.5, 32)
    scale = g / np.sqrt(rv + O.BN_EPS)
    return (g, b, rm, rv), cu(scale), cu(b - rm * scale)


def _ints(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)


# ---- conv1 --------------------------------------------------------------------------------------------------------------------
# (chunk frames, window offset, output frames, ragged): J = 0, 1, 63, 64, 65 around the 64-frame tile, offsets 0 / 1 and the
# start-of-stream 5, a chunk shorter than the carry, a 1-frame chunk whose frame reads beyond the chunk, a ragged end
CONV1_FEEDS = [(3, 5, 0, False), (1, 1, 1, False), (130, 0, 63, False), (131, 1, 64, False), (133, 0, 65, True), (3, 1, 2, False)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("F0", [161, 81])
def test_stream_conv1_chain_of_feeds(F0, N, dtype):
    from deepspeech.pytorch_amd import ops
    rng = np.random.default_rng(F0 + N)
    w = rng.normal(0, 1 / np.sqrt(451), (32, 1, 41, 11)).astype(np.float32).astype(np.float64)
    b = rng.normal(0, 0.1, 32).astype(np.float32).astype(np.float64)
    _, scale, shift = _bn(rng)
    w1k, b1 = cu(w.reshape(32, 451).T), cu(b)
    carry = [torch.zeros((N, F0, K), device=DEV), torch.full((N, F0, K), 7.0, device=DEV)]
    ref_carry, cur = np.zeros((N, 1, F0, K)), 0
    for Tc, off, J, ragged in CONV1_FEEDS:
        x = rng.standard_normal((N, 1, F0, Tc)).astype(np.float32)
        lens = [Tc, Tc - 3, Tc - 11][:N] if ragged else [Tc] * N
        live = [J, J - 2, J - 5][:N] if ragged else [J] * N
        v, ref_carry = window(ref_carry, x.astype(np.float64), lens, 3)
        # folded epilogue == eval BatchNorm with these statistics: gamma' = scale, beta' = shift, mean 0, var 1 - eps
        want = conv_window(v, off, J, w, b, np64(scale), np64(shift), np.zeros(32), np.full(32, 1.0 - O.BN_EPS), 2, live)
        old = carry[cur].clone()
        y = ops.stream_conv1(cu(x), carry[cur], carry[1 - cur], w1k, b1, scale, shift, off, J, dtype,
                             lens=_ints(lens) if ragged else None, live=_ints(live) if ragged else None)
        assert torch.equal(carry[cur], old)                                     # the old carry is only read
        assert torch.equal(carry[1 - cur], cu(ref_carry[:, 0])), (Tc, off, J)   # next carry = the window's tail, exactly
        cur ^= 1
        got = np64(y).transpose(0, 3, 1, 2)                                     # [N][F1][J][32] -> (N, 32, F1, J)
        assert got.shape == want.shape
        if J:
            e = relerr(got, want)
            print("conv1 F0=%d N=%d %s feed %s: relerr %.2e" % (F0, N, dtype, (Tc, off, J), e))
            assert e <= TOL[dtype]
            for n in range(N):
                assert not got[n, :, :, live[n]:].any()                         # masked frames are zeros


# ---- conv2 --------------------------------------------------------------------------------------------------------------------
# (new activation frames, window offset, output frames, ragged): J = 0, 1, 31, 32, 33 around the 32-position tile, the
# start-of-stream offsets 5 .. 1 (fewer than 5 conv1 frames before the feed), a ragged end, frames that read beyond the window
CONV2_FEEDS = [(3, 5, 0, False), (4, 2, 1, False), (31, 0, 31, False), (32, 0, 32, False), (33, 0, 33, True), (2, 3, 5, False),
               (6, 4, 3, False), (5, 1, 2, False)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("F0", [161, 81])
def test_stream_conv2_chain_of_feeds(F0, N, dtype):
    from deepspeech.pytorch_amd import ops
    rng = np.random.default_rng(F0 + N)
    F1, F2 = ops.conv_rows(F0)
    rin, rld = 32 * F2, (32 * F2 + 63) // 64 * 64
    assert rld > rin                                                            # both geometries have pad columns
    w = rnd(rng.normal(0, 1 / np.sqrt(32 * 21 * 11), (32, 32, 21, 11)), dtype)
    b = rng.normal(0, 0.1, 32).astype(np.float32).astype(np.float64)
    _, scale, shift = _bn(rng)
    w2t, b2 = cu(w.transpose(2, 3, 0, 1), dtype), cu(b)
    carry = [torch.zeros((N, F1, K, 32), device=DEV, dtype=dtype), torch.full((N, F1, K, 32), 7.0, device=DEV, dtype=dtype)]
    ref_carry, cur = np.zeros((N, 32, F1, K)), 0
    for Jin, off, J, ragged in CONV2_FEEDS:
        a1 = rnd(rng.uniform(0, 4, (N, 32, F1, Jin)), dtype)                    # post-Hardtanh activations as stored
        live = [J, J - 3, J - 16][:N] if ragged else [J] * N
        v, ref_carry = window(ref_carry, a1, [Jin] * N, 3)
        want = conv_window(v, off, J, w, b, np64(scale), np64(shift), np.zeros(32), np.full(32, 1.0 - O.BN_EPS), 1, live)
        old = carry[cur].clone()
        x0 = torch.full((J * N, rld), 7.0, device=DEV, dtype=dtype)
        ops.stream_conv2(cu(a1.transpose(0, 2, 3, 1), dtype), carry[cur], carry[1 - cur], w2t, b2, scale, shift, off, J, rld, F0=F0,
                         live=_ints(live) if ragged else None, out=x0)
        assert torch.equal(carry[cur], old)
        assert torch.equal(carry[1 - cur], cu(ref_carry.transpose(0, 2, 3, 1), dtype)), (Jin, off, J)
        cur ^= 1
        got = np64(x0).reshape(J, N, rld)
        assert not got[:, :, rin:].any()                                        # the zero pad columns of the sequence layout
        if J:
            feat = got[:, :, :rin].reshape(J, N, F2, 32).transpose(1, 3, 2, 0)  # feature f*32 + c -> (N, 32, F2, J)
            e = relerr(feat, want)
            print("conv2 F0=%d N=%d %s feed %s: relerr %.2e" % (F0, N, dtype, (Jin, off, J), e))
            assert e <= TOL[dtype]
            for n in range(N):
                assert not feat[n, :, :, live[n]:].any()


# ---- lookahead ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [16, 64, "padded 50"])
@pytest.mark.parametrize("ctx", [1, 3, 20, 40])
def test_stream_lookahead_chain_of_feeds(ctx, H, dtype):
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd.model import _padded_hidden
    Ht = 50 if H == "padded 50" else H
    H = _padded_hidden(50, "gru", 32, False) if H == "padded 50" else H          # the internal width of a 50-unit model
    assert H >= Ht and H % 16 == 0
    N, rng = 3, np.random.default_rng(ctx + H)
    w = np.zeros((H, 1, ctx))
    w[:Ht] = rng.normal(0, 1 / np.sqrt(ctx), (Ht, 1, ctx)).astype(np.float32)
    wd = cu(w[:, 0])
    carry = [torch.zeros((ctx - 1, N, H), device=DEV, dtype=dtype), torch.full((ctx - 1, N, H), 7.0, device=DEV, dtype=dtype)]
    ref_carry, cur = np.zeros((ctx - 1, N, H)), 0
    # (new rows, window offset, output rows, ragged): the start of a stream (nothing carried yet, reads beyond the chunk), then
    # J = 16 and 17 around the 16-frame block of the one-shot kernel, the last with streams that ended earlier
    for Jin, off, J, ragged in [(5, ctx - 1, 1, False), (16, 0, 16, False), (17, 0, 17, True), (2, 0, 3, False)]:
        x = rnd(rng.uniform(-1, 1, (Jin, N, H)) * (np.arange(H) < Ht), dtype)
        lens = [Jin, Jin - 2, Jin - 8] if ragged else [Jin] * N
        v, ref_carry = window(ref_carry, x, lens, 0)
        want = lookahead_window(v, off, J, w)
        old = carry[cur].clone()
        y = ops.stream_lookahead(cu(x.reshape(Jin * N, H), dtype), carry[cur] if ctx > 1 else None, carry[1 - cur] if ctx > 1 else None, wd,
                                 N, H, off, J, lens=_ints(lens) if ragged else None)
        if ctx > 1:
            assert torch.equal(carry[cur], old)
            assert torch.equal(carry[1 - cur], cu(ref_carry, dtype)), (Jin, off, J)
            cur ^= 1
        got = np64(y).reshape(J, N, H)
        e = relerr(got, want)
        print("lookahead ctx=%d H=%d %s feed %s: relerr %.2e" % (ctx, H, dtype, (Jin, off, J), e))
        assert e <= TOL[dtype]
        assert not got[:, :, Ht:].any()                                         # the padded units stay exactly 0


# ---- model level --------------------------------------------------------------------------------------------------------------
def _stream(m, dec, x, lengths, chunks, **kw):
    """Feeds x (N, 1, F0, T) in `chunks` + the rest (final, ragged by `lengths`) through an exact session.  Returns (the emitted
    probabilities per stream, concatenated [N] (frames, C) fp64 arrays; per feed (text, (probs, sizes) or None); the session)."""
    from deepspeech.pytorch_amd.streaming import StreamingTranscriber
    N, T = x.shape[0], x.shape[3]
    st = StreamingTranscriber(m, dec, carry_context=True, **kw)
    chunks = list(chunks) + [T - sum(chunks)]
    assert chunks[-1] > 0 and min(lengths) > T - chunks[-1]                     # every stream ends in the final feed
    per_feed, got, pos = [], [[] for _ in range(N)], 0
    for i, c in enumerate(chunks):
        last = i == len(chunks) - 1
        lens = [int(g) - pos for g in lengths] if last else [c] * N
        text = st.feed(x[:, :, :, pos:pos + c].contiguous(), lens, final=last)
        per_feed.append((text, st.last_output))
        if st.last_output is not None:
            probs, sizes = st.last_output
            for n in range(N):
                got[n].append(np64(probs[n, :sizes[n]]))
        pos += c
    C_ = len(m.labels)
    return [np.concatenate(g) if g else np.zeros((0, C_)) for g in got], per_feed, st


def _check_counts(per_feed, chunks_all, ctx):
    from deepspeech.pytorch_amd.streaming import plan_feed
    G = 0
    for i, ((_, out), c) in enumerate(zip(per_feed, chunks_all)):
        p = plan_feed(G, c, ctx, final=(i == len(chunks_all) - 1))
        assert (0 if out is None else out[0].shape[1]) == p.j3_new - p.j3_old, (i, c)
        G += c


FIXTURE_CASES = [("gru_uni_la", None, CHUNKS), ("gru_uni_h50_la40_c45", None, CHUNKS), ("lstm_uni_la", None, CHUNKS[:2]),
                 ("lstm_uni_la", 1, CHUNKS)]
_ORACLE = {}


def _fixture_case(name, N):
    """(fixture, inputs on the device, lengths, fp64 oracle eval probabilities), the oracle computed once per case"""
    fx = Fixture(name)
    inputs = fx.batch()[0]
    lengths = [int(v) for v in fx.z["input_sizes"]]
    if N is not None:
        lengths = lengths[:N]
        inputs = inputs[:N, :, :, :lengths[0]]
    key = (name, N)
    if key not in _ORACLE:
        P = {k: v.astype(np.float64) for k, v in fx.params().items()}
        _ORACLE[key] = O.model_forward(P, fx.cfg, inputs.astype(np.float64), np.asarray(lengths), train=False, keep_cache=False)[:2]
    return fx, torch.from_numpy(np.ascontiguousarray(inputs)).to(DEV), lengths, _ORACLE[key]


def _synth_case():
    """160 frames, 2 streams, gru_uni_la's weights: long enough for a ctx = 20 model to emit in the middle of the stream"""
    from deepspeech.pytorch_amd import synth
    fx = Fixture("gru_uni_la")
    lengths = [160, 155]
    inputs = synth.synth_batch(np.asarray(lengths), seed=11)[0]
    if "synth" not in _ORACLE:
        P = {k: v.astype(np.float64) for k, v in fx.params().items()}
        _ORACLE["synth"] = O.model_forward(P, fx.cfg, inputs.astype(np.float64), np.asarray(lengths), train=False, keep_cache=False)[:2]
    return fx, torch.from_numpy(inputs).to(DEV), lengths, _ORACLE["synth"]


SYNTH_CHUNKS = (54, 1, 2, 37)                           # then 66: the first feed is exactly the model's latency


def _max_err(got, ref, out_lens):
    return max(np.abs(got[n] - ref[n, :out_lens[n]]).max() for n in range(len(got)))


@pytest.mark.parametrize("name,N,chunks", FIXTURE_CASES)
def test_fp32_streamed_fixture_matches_the_golden_eval_probs(name, N, chunks):
    from deepspeech.pytorch_amd import decoder as D
    fx, x, lengths, _ = _fixture_case(name, N)
    m = build(fx, 32).eval()
    got, per_feed, st = _stream(m, D.GreedyDecoder(fx.labels), x, lengths, chunks)
    out_lens = fx.z["output_lengths"]
    gold = fx.z["eval_probs"].astype(np.float64)
    for n in range(len(lengths)):
        assert got[n].shape[0] == out_lens[n] == st.frames[n]
    err = _max_err(got, gold, out_lens)
    print("%s N=%s %s: streamed vs golden eval_probs %.2e" % (name, N, chunks, err))
    assert err <= 1e-4
    _check_counts(per_feed, list(chunks) + [x.shape[3] - sum(chunks)], fx.cfg["lookahead_context"])


def test_fp32_streamed_160_frames_emit_mid_stream_and_match_the_oracle():
    from deepspeech.pytorch_amd import decoder as D
    fx, x, lengths, (ref, out_lens) = _synth_case()
    m = build(fx, 32).eval()
    got, per_feed, st = _stream(m, D.GreedyDecoder(fx.labels), x, lengths, SYNTH_CHUNKS)
    assert st.latency_frames == SYNTH_CHUNKS[0] and per_feed[0][1][0].shape[1] == 1          # the first feed emits exactly 1 frame
    assert per_feed[1][1] is None and sum(o is not None for _, o in per_feed) >= 3           # ... the 1-frame feed nothing
    assert [g.shape[0] for g in got] == [int(v) for v in out_lens]
    err = _max_err(got, ref, out_lens)
    print("synth 160: streamed vs oracle %.2e" % err)
    assert err <= 1e-4
    _check_counts(per_feed, list(SYNTH_CHUNKS) + [160 - sum(SYNTH_CHUNKS)], 20)


@pytest.mark.parametrize("case", ["gru_uni_la", "gru_uni_h50_la40_c45", "lstm_uni_la", "synth"])
def test_bf16_streamed_is_no_worse_than_twice_the_one_shot_bf16_forward(case):
    """The folded epilogue rounds a conv output once where the one-shot rounds twice, so single elements move by a bf16 ulp either
    way: the streamed error against the fp64 oracle may be up to twice the one-shot bf16 forward's own."""
    from deepspeech.pytorch_amd import decoder as D
    if case == "synth":
        (fx, x, lengths, (ref, out_lens)), chunks = _synth_case(), SYNTH_CHUNKS
    else:
        (fx, x, lengths, (ref, out_lens)), chunks = _fixture_case(case, None), (CHUNKS[:2] if case == "lstm_uni_la" else CHUNKS)
    m = build(fx, "bf16").eval()
    with torch.no_grad():
        one = np64(m(x, torch.tensor(lengths, dtype=torch.int))[0])
    e_oneshot = _max_err([one[n, :out_lens[n]] for n in range(len(lengths))], ref, out_lens)
    got, _, _ = _stream(m, D.GreedyDecoder(fx.labels), x, lengths, chunks)
    e_stream = _max_err(got, ref, out_lens)
    print("%s bf16: e_stream %.3e, e_oneshot %.3e" % (case, e_stream, e_oneshot))
    assert e_stream <= 2 * e_oneshot


# ---- session ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["greedy", "beam"])
def test_session_transcripts_follow_the_emitted_frames_and_reset_repeats_them(kind):
    from deepspeech.pytorch_amd import decoder as D
    fx, x, lengths, _ = _synth_case()
    m = build(fx, 32).eval()
    dec = D.GreedyDecoder(fx.labels) if kind == "greedy" else D.BeamCTCDecoder(fx.labels, beam_width=8)
    _, per_feed, st = _stream(m, dec, x, lengths, SYNTH_CHUNKS, max_frames=80)
    N, rows = len(lengths), [[] for _ in lengths]
    for text, out in per_feed:
        if out is not None:
            for n in range(N):
                rows[n].append(out[0][n, :out[1][n]])
        sizes = torch.tensor([sum(r.shape[0] for r in rows[n]) for n in range(N)], dtype=torch.int)
        if int(sizes.max()) == 0:
            assert text == [''] * N
            continue
        pad = torch.zeros((N, int(sizes.max()), len(fx.labels)), device=DEV)
        for n in range(N):
            pad[n, :int(sizes[n])] = torch.cat(rows[n])
        strings, offsets = dec.decode(pad, sizes)
        assert text == [s[0] for s in strings]                                  # the transcript after every feed, exactly
    assert st.frames == sizes.tolist() and any(per_feed[-1][0])
    got = st.finish()
    assert got[0] == strings and all(torch.equal(a, b) for u, v in zip(got[1], offsets) for a, b in zip(u, v))
    with pytest.raises(ValueError, match="ended"):
        st.feed(x[:, :, :, :5].contiguous(), [5, 5])                            # after the end, until reset()
    st.reset()
    assert st.hs is None and st.frames == [0] * N
    pos = 0
    for (text, out), c in zip(per_feed[:3], SYNTH_CHUNKS[:3]):                  # the first feeds again: bit for bit
        assert st.feed(x[:, :, :, pos:pos + c].contiguous(), [c] * N) == text
        assert (st.last_output is None) == (out is None)
        if out is not None:
            assert torch.equal(st.last_output[0], out[0]) and st.last_output[1] == out[1]
        pos += c
    assert st.end() == st.best() and st.frames == [int(v) for v in O.seq_lens([pos] * N)]
    with pytest.raises(ValueError, match="ended"):
        st.feed(x[:, :, :, :5].contiguous(), [5, 5])                            # ... and after end() as well


def test_default_mode_is_untouched_and_a_bidirectional_model_is_refused():
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.streaming import StreamingTranscriber
    from test_gpu_streaming import _chunks, _concat, _loop
    fx = Fixture("lstm_uni_la")
    m = build(fx, 32).eval()
    chunks = _chunks(fx, 2)
    outs = _loop(m, chunks)
    dec = D.GreedyDecoder(fx.labels)
    st = StreamingTranscriber(m, dec)
    assert not st.carry_context and st.latency_frames == 0
    for i, (x, lens) in enumerate(chunks):
        text = st.feed(x, lens)
        probs, sizes = _concat(outs, i + 1)
        assert st.frames == sizes.tolist() and text == [s[0] for s in dec.decode(probs, sizes)[0]]
    with pytest.raises(ValueError, match="carry_context"):
        st.feed(*chunks[0], final=True)
    bi = Fixture("gru_bi_tiny")
    with pytest.raises(ValueError, match="uni-directional"):
        StreamingTranscriber(build(bi, 32), D.GreedyDecoder(bi.labels), carry_context=True)
