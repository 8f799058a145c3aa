"""GPU checks of the running (causal) normalisation of the spectrogram front-end and of its streaming form (DESIGN.md section
3.6.4; csrc/ds2_spect.hip: k_spect_frame_stats, k_spect_scan, k_spect_write<., true>, k_spect_stream_window / _carry;
SpectrogramFrontEnd(normalize="running"), SpectStream, StreamingTranscriber.feed_wave, StreamPool.feed_wave).

Bounds: the one-shot running call against the fp64 restatement (tests/spect_stream_reference.py on the oracle's raw
log-magnitudes) is held to 2e-4, the bound tests/test_gpu_spect.py holds the front-end to; with SpecAugment to the bound of
tests/test_gpu_spec_augment.py; the streamed model against the one-shot eval forward and the pool against the single-stream
session to 1e-4 (tests/test_gpu_stream_exact.py, tests/test_gpu_stream_pool.py).  Everything between the streaming form and
the one-shot call is torch.equal: the strict fp64 fold and the position-independent GEMM rows make the chunking invisible."""
import numpy as np
import pytest
import torch

import spec_augment_reference as R
import spect_stream_reference as SR
from fixtures import DEV, Fixture, np64
from oracle import ds2_oracle as O
from test_gpu_model import build
from test_gpu_spec_augment import bound, noise as specaug_noise
from test_spect_stream_host import cases

pytestmark = pytest.mark.gpu
HOP, NBIN = 160, 161
PATTERN = 0xA5


def front_end(normalize="running", pad_mode="constant", **kw):
    from deepspeech.pytorch_amd import configs
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    return SpectrogramFrontEnd(configs.SpectConfig(), normalize=normalize, pad_mode=pad_mode, **kw)


def clip(seed, n, scale=0.1):
    return (np.random.RandomState(seed).standard_normal(n) * scale).astype(np.float32)


def pack(wavs, width=None):
    buf = torch.zeros((len(wavs), width or max(len(w) for w in wavs)))
    for i, w in enumerate(wavs):
        buf[i, :len(w)] = torch.from_numpy(w)
    return buf.to(DEV)


def restated(w, pad_mode="constant", **kw):
    return SR.running_normalize(O.log_spectrogram(w.astype(np.float64), normalize=False, pad_mode=pad_mode), **kw)


# ---- 1. the one-shot running call against the fp64 restatement ------------------------------------------------------------------
@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 257])
def test_one_shot_running_matches_the_restatement(T, pad_mode):
    """a ragged batch of 3 whose longest clip has T frames"""
    lens = sorted({(T - 1) * HOP + 37, max((T - 1) * HOP // 2, 2), 1}, reverse=True)
    lens = (lens + [1, 1])[:3]
    wavs = [clip(10 * T + k, n) + 0.01 for k, n in enumerate(lens)]
    out, pct, frames = front_end(pad_mode=pad_mode)(pack(wavs), lens)
    assert tuple(out.shape) == (3, 1, NBIN, T) and frames.tolist() == [1 + n // HOP for n in lens]
    got = np64(out)
    worst = 0.0
    for i, w in enumerate(wavs):
        ref = restated(w, pad_mode)
        Ti = ref.shape[1]
        worst = max(worst, float(np.abs(got[i, 0, :, :Ti] - ref).max()))
        assert np.all(got[i, 0, :, Ti:] == 0)
    print("running T=%d %s: max |device - f64| = %.3e" % (T, pad_mode, worst))
    assert np.isfinite(got).all() and worst < 2e-4


def test_leading_silence_gives_zeros_and_no_nan():
    w = clip(5, 8000)
    w[:1600] = 0.0                                                    # 0.1 s of digital silence: frames 0..8 see zeros only
    out = np64(front_end()(pack([w]), [8000])[0])[0, 0]
    assert np.isfinite(out).all() and np.all(out[:, :9] == 0) and np.abs(out[:, 10:]).max() > 0.1
    assert np.abs(out - restated(w)).max() < 2e-4


def test_prior_shifts_the_first_frames_as_the_restatement_says():
    w = clip(6, 4000)
    prior = (0.05, 0.04, 30)
    plain = np64(front_end()(pack([w]), [4000])[0])[0, 0]
    got = np64(front_end(running_prior=prior, running_floor=1e-3)(pack([w]), [4000])[0])[0, 0]
    assert np.abs(got - restated(w, prior=prior, floor=1e-3)).max() < 2e-4
    assert np.abs(got[:, 0] - plain[:, 0]).max() > 1e-2               # frame 0: 161 values against 161 + 30 * 161


# ---- 2. streaming == one-shot, bit for bit --------------------------------------------------------------------------------------
_ONE_SHOT = {}


def one_shot(lens, seed, normalize="running"):
    """the clips (seeded by their lengths) and their one-shot spectrograms as a batch, computed once"""
    key = (tuple(lens), seed, normalize)
    if key not in _ONE_SHOT:
        wavs = [clip(seed + 7 * k + n, n) for k, n in enumerate(lens)]
        out, _, frames = front_end(normalize)(pack(wavs), lens)
        _ONE_SHOT[key] = (wavs, out.clone(), frames.tolist())
    return _ONE_SHOT[key]


def stream_clips(stream, slots, wavs, feeds, frames_out=None):
    """feeds: [(per-row sample counts, final)].  Returns per row the concatenated frames (161, T) on the device."""
    pos, got = [0] * len(wavs), [[] for _ in wavs]
    for counts, final in feeds:
        width = max(counts)
        chunk = pack([w[p:p + c] for w, p, c in zip(wavs, pos, counts)], width) if width else torch.zeros((len(wavs), 0), device=DEV)
        out, frames = stream.feed(slots, chunk, counts, final=slots if final else ())
        assert tuple(out.shape) == (len(wavs), 1, NBIN, max(frames))
        for r, f in enumerate(frames):
            assert not out[r, 0, :, f:].any()                        # frames beyond the row's own count are zero
            got[r].append(out[r, 0, :, :f])
            pos[r] += counts[r]
        if frames_out is not None:
            frames_out.append(frames)
    return [torch.cat(g, 1) for g in got]


def lockstep_feeds(lens, chunk, flush_only=False):
    """all rows bring `chunk` samples (None: everything at once) while every row has more than that left, an empty feed in front
    of every third; then the ragged final feed -- or the rest in a feed that is not final and a flush-only final feed."""
    feeds, pos, k = [], 0, 0
    if chunk is not None:
        while min(lens) - pos > chunk:
            if k % 3 == 0:
                feeds.append(([0] * len(lens), False))
            feeds.append(([chunk] * len(lens), False))
            pos, k = pos + chunk, k + 1
    rest = [n - pos for n in lens]
    return feeds + ([(rest, False), ([0] * len(lens), True)] if flush_only else [(rest, True)])


@pytest.mark.parametrize("L,chunk", cases())
def test_streaming_equals_the_one_shot_call(L, chunk):
    """3 streams of L + 171, L + 40 and L samples in lock step, a non-final feed of 0 samples in front of every third feed, a
    ragged final feed"""
    lens = [L + 171, L + 40, L]
    wavs, ref, frames = one_shot(lens, 100)
    got = stream_clips(front_end().stream(3, DEV), [0, 1, 2], wavs, lockstep_feeds(lens, chunk))
    for r, T in enumerate(frames):
        assert got[r].shape[1] == T and torch.equal(got[r], ref[r, 0, :, :T]), (r, float((got[r] - ref[r, 0, :, :T]).abs().max()))


@pytest.mark.parametrize("L", [1, 160, 321, 2037])
def test_flush_only_final_feed_and_raw_log_magnitudes(L):
    """every sample in feeds that are not final, then a final feed of 0 samples (one frame from the carry alone); the same with
    normalize=False; and slots given out of order on a larger stream"""
    lens = [L + 171, L + 40, L]
    for normalize in ("running", False):
        wavs, ref, frames = one_shot(lens, 100, normalize)
        per_feed = []
        got = stream_clips(front_end(normalize).stream(5, DEV), [4, 0, 2], wavs, lockstep_feeds(lens, 161, flush_only=True), per_feed)
        assert per_feed[-1] == [1, 1, 1]
        for r, T in enumerate(frames):
            assert torch.equal(got[r], ref[r, 0, :, :T])


# ---- 3. slot reuse --------------------------------------------------------------------------------------------------------------
def test_a_reused_slot_starts_fresh():
    wavs, ref, frames = one_shot([2037, 1000], 300)
    st = front_end().stream(2, DEV)
    stream_clips(st, [0, 1], [clip(1, 900, 0.7) + 0.3] * 2, [([333, 333], False), ([333, 100], False)])      # mid-utterance, loud, offset
    st.reset([1])
    got = stream_clips(st, [1], [wavs[0]], [([7], False), ([1000], False), ([1030], True)])[0]
    assert torch.equal(got, ref[0, 0, :, :frames[0]])
    with pytest.raises(ValueError, match="ended"):
        st.feed([1], torch.zeros((1, 4), device=DEV), [4])
    st.reset()                                                       # all slots; the other one was left mid-utterance
    got = stream_clips(st, [0, 1], wavs, [([500, 500], False), ([1537, 500], True)])
    assert torch.equal(got[0], ref[0, 0, :, :frames[0]]) and torch.equal(got[1], ref[1, 0, :, :frames[1]])


# ---- 4. normalize=True / False are what they were -------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_per_utterance_and_raw_modes_equal_the_direct_call(pad_mode, normalize):
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd._lib import call, query
    lens = [10240, 801, 159]
    fe = front_end(normalize, pad_mode)
    wav = pack([clip(40 + k, n) for k, n in enumerate(lens)])
    got, _, _ = fe(wav, lens)
    N, Lm = 3, max(lens)
    out = torch.empty((N, 1, NBIN, 1 + Lm // HOP), dtype=torch.float32, device=DEV)
    ws = torch.empty(query("ds2_spect_ws_bytes", N, Lm), dtype=torch.uint8, device=DEV)
    ns = torch.tensor(lens, dtype=torch.int32, device=DEV)
    call("ds2_spectrogram", ops.P(wav), wav.stride(0), ops.P(ns), N, Lm, ops.P(fe._basis_on(wav.device)), int(pad_mode == "reflect"),
         int(normalize), ops.P(out), ops.P(ws), ops.S())
    assert torch.equal(got, out)
    if not normalize:                                                # the streaming kernels' raw path is the same raw value
        raw = front_end(False, pad_mode)(wav, lens)[0]
        assert torch.equal(raw, out)


# ---- 5. SpecAugment on the running normalisation --------------------------------------------------------------------------------
def test_augment_with_running_normalisation_matches_the_restatement():
    """T = 65, 64, 12.  The warp interpolates frames that carry their own statistics and its control value is the normalised
    centre bin of frame i: the restatement warps the running-normalised spectrogram.  Two comparisons, with the coefficients the
    device used (checked apart: their control value is an fp32 device value): against the fp64 warp of the DEVICE's own plain
    running spectrogram at the bound of tests/test_gpu_spec_augment.py, as that file compares; and against the restatement from
    the oracle's log-magnitudes at that bound plus the 2e-4 the plain front-end is allowed (a lerp is a convex combination, so the
    plain output's error passes through undiminished at most).  The seed is the first whose flows stay moderate on every clip."""
    from deepspeech.pytorch_amd.augment import SpecAugment
    lens = [64 * HOP, 63 * HOP + 7, 11 * HOP + 5]
    frames = [1 + n // HOP for n in lens]
    wavs = [clip(70 + k, n, 0.05 + 0.2 * k) for k, n in enumerate(lens)]
    sa = SpecAugment(frequency_mask_num=2, time_mask_num=2, time_masking_para=20, W=5)
    raws = [O.log_spectrogram(w.astype(np.float64), normalize=False, pad_mode="constant") for w in wavs]
    xs = [SR.running_normalize(r) for r in raws]
    for seed in range(1000):
        warp, fm, tm = sa.draw(frames, NBIN, np.random.default_rng(seed))
        cfs = [R.warp_coef(NBIN, T, xs[k][80, max(int(warp[k, 0]), 0)], int(warp[k, 0]), int(warp[k, 1]), warp[k, 2:11]) for k, T in enumerate(frames)]
        if all(c.any() and np.abs(c) @ np.array([160.0, T - 1, 1.0]) <= 2 * T for c, T in zip(cfs, frames)):
            break
    else:
        raise AssertionError("no draw found")
    fe = front_end(spec_augment=sa, rng=np.random.default_rng(seed))
    wav = pack(wavs)
    plain = np64(front_end()(wav, lens)[0])
    fused = np64(fe(wav, lens, augment=True)[0])
    coef = np64(fe.last_coef)
    for k, T in enumerate(frames):
        assert np.allclose(coef[k], cfs[k], rtol=1e-4, atol=1e-6), (k, coef[k], cfs[k])
        allowed = bound(specaug_noise()["e2e_f161_t%d" % T], xs[k])
        err_dev = float(np.abs(fused[k, 0, :, :T] - R.spec_augment(plain[k, 0, :, :T], coef[k], fm[k], tm[k])).max())
        err64 = float(np.abs(fused[k, 0, :, :T] - SR.spec_augment_running(raws[k], coef[k], fm[k], tm[k])).max())
        print("clip %d (T %d): |fused - f64 warp of the device's plain| %.3e allowed %.3e, |fused - f64| %.3e" % (k, T, err_dev, allowed, err64))
        assert err_dev <= allowed and err64 <= 2e-4 + allowed
        assert np.all(fused[k, 0, :, T:] == 0) and np.all(fused[k, 0, :, :T][R.in_mask(NBIN, T, fm[k], tm[k])] == 0)
        assert np.any(fused[k, 0, :, :T] != plain[k, 0, :, :T])


def test_wave_augment_and_collate_take_the_running_mode():
    from deepspeech.pytorch_amd.augment import WaveAugment
    waves = [torch.from_numpy(clip(80 + k, n)) for k, n in enumerate((4000, 9000, 480))]
    inputs, pct, order = front_end().collate(waves)
    assert order == [1, 0, 2]
    for r, i in enumerate(order):
        ref = restated(waves[i].numpy())
        assert np.abs(np64(inputs)[r, 0, :, :ref.shape[1]] - ref).max() < 2e-4
    fe = front_end(wave_augment=WaveAugment(speed_volume_perturb=True), rng=np.random.default_rng(2))
    out, _, frames = fe(pack([w.numpy() for w in waves]), [4000, 9000, 480])
    assert torch.isfinite(out).all() and frames.tolist() == [1 + int(n) // HOP for n in fe.last_wave[0].nsamples]
    assert all(bool(out[i, 0, :, :f].any()) and not bool(out[i, 0, :, f:].any()) for i, f in enumerate(frames.tolist()))
    with pytest.raises(ValueError, match="wave_augment"):
        fe.stream(1, DEV)


# ---- 6. model level -------------------------------------------------------------------------------------------------------------
WAVE_LENS = [16037, 15500]


@pytest.fixture(scope="module")
def model_case():
    """gru_uni_la's weights, two streams of 0.1 * randn, their one-shot running spectrogram and the one-shot eval forward"""
    fx = Fixture("gru_uni_la")
    m = build(fx, 32).eval()
    rs = np.random.RandomState(17)
    wavs = [(0.1 * rs.standard_normal(n)).astype(np.float32) for n in WAVE_LENS]
    spect, _, frames = front_end()(pack(wavs), WAVE_LENS)
    with torch.no_grad():
        probs, out_lens, _ = m(spect, frames.to(torch.int))
    return fx, m, wavs, spect, frames.tolist(), np64(probs), [int(v) for v in out_lens]


def wave_session(m, fx, wavs, chunk):
    """feed_wave in `chunk`-sample feeds while both streams have more than that left, then the ragged final feed.  Returns
    (per stream the emitted probabilities [tensor], per feed (input frames completed so far, last_output or None), session)."""
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.streaming import StreamingTranscriber
    st = StreamingTranscriber(m, D.GreedyDecoder(fx.labels), carry_context=True)
    pos, got, per_feed = 0, [[], []], []
    while True:
        final = min(WAVE_LENS) - pos <= chunk
        counts = [n - pos for n in WAVE_LENS] if final else [chunk, chunk]
        st.feed_wave(pack([w[pos:pos + c] for w, c in zip(wavs, counts)]), counts, final=final)
        pos += chunk
        per_feed.append((pos // HOP if not final else None, st.last_output))
        if st.last_output is not None:
            for n in range(2):
                got[n].append(st.last_output[0][n, :st.last_output[1][n]])
        if final:
            return got, per_feed, st


def test_feed_wave_in_whole_frames_equals_the_session_fed_the_one_shot_spectrogram(model_case):
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.streaming import StreamingTranscriber
    fx, m, wavs, spect, frames, _, _ = model_case
    got, per_feed, st = wave_session(m, fx, wavs, 3200)
    ref = StreamingTranscriber(m, D.GreedyDecoder(fx.labels), carry_context=True)
    pos, want = 0, [[], []]
    for k in range(len(per_feed)):
        final = k == len(per_feed) - 1
        lens = [f - pos for f in frames] if final else [20, 20]
        ref.feed(spect[:, :, :, pos:pos + max(lens)].contiguous(), lens, final=final)
        pos += 20
        assert (ref.last_output is None) == (per_feed[k][1] is None)
        if ref.last_output is not None:
            for n in range(2):
                want[n].append(ref.last_output[0][n, :ref.last_output[1][n]])
    for n in range(2):
        assert torch.equal(torch.cat(got[n]), torch.cat(want[n]))
    assert st.best() == ref.best() and st.finish() is not None and st.frames == ref.frames


def test_feed_wave_in_333_sample_feeds_matches_the_one_shot_forward(model_case):
    from deepspeech.pytorch_amd.spectrogram import plan_wave
    from deepspeech.pytorch_amd.streaming import plan_feed
    fx, m, wavs, _, frames, probs, out_lens = model_case
    got, per_feed, st = wave_session(m, fx, wavs, 333)
    err = 0.0
    for n in range(2):
        g = np64(torch.cat(got[n]))
        assert g.shape[0] == out_lens[n] == st.frames[n]
        err = max(err, float(np.abs(g - probs[n, :out_lens[n]]).max()))
    print("feed_wave(333): streamed vs one-shot forward %.2e" % err)
    assert err <= 1e-4
    G, F, first = 0, 0, None
    for k, (_, out) in enumerate(per_feed):
        final = k == len(per_feed) - 1
        e = max(plan_wave(G, (n - G) if final else 333, final).emit for n in WAVE_LENS)
        p = plan_feed(F, e, 20, final)
        assert (0 if out is None else out[0].shape[1]) == p.j3_new - p.j3_old, k
        if out is not None and first is None:
            first = (F, F + e)
        G, F = G + 333, F + e
    assert st.latency_frames == 54 and first[0] < 54 <= first[1]       # the feed that completes input frame 54


# ---- 7. the pool ----------------------------------------------------------------------------------------------------------------
def test_pool_feed_wave_rows_of_any_lengths(model_case):
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.streaming import StreamPool, StreamingTranscriber
    fx, m = model_case[:2]
    dec = D.GreedyDecoder(fx.labels)
    rs = np.random.RandomState(23)
    clips = {"a": 13480, "b": 9037, "c": 9100}
    clips = {k: (0.1 * rs.standard_normal(n)).astype(np.float32) for k, n in clips.items()}
    pool = StreamPool(m, dec, 3)
    got = {k: [] for k in clips}

    def feed(names, slots, counts, pos, final=()):
        width = max(counts)
        chunk = pack([clips[k][p:p + c] for k, p, c in zip(names, pos, counts)], width) if width else torch.zeros((len(names), 0), device=DEV)
        pool.feed_wave([slots[k] for k in names], chunk, counts, final=[slots[k] for k in final])
        for k in names:
            if slots[k] in pool.last_output:
                got[k].append(pool.last_output[slots[k]])

    slots = {"a": pool.open(), "b": pool.open()}
    feed(["a", "b"], slots, [9000, 9000], [0, 0])
    slots["c"] = pool.open()
    feed(["a", "c", "b"], slots, [480, 100, 37], [9000, 0, 9000], final=["b"])        # 3 frames, no frame, the final row
    assert pool._wave.frames(slots["c"]) == 0 and pool._wave.frames(slots["b"]) == 1 + 9037 // HOP
    feed(["c", "a"], slots, [9000, 4000], [100, 9480])
    with pytest.raises(ValueError, match="ended"):
        pool.feed_wave([slots["b"]], torch.zeros((1, 8), device=DEV), [8])
    text = pool.end([slots["a"], slots["c"]])
    for k in ("a", "c"):
        if slots[k] in pool.last_output:
            got[k].append(pool.last_output[slots[k]])
    worst = 0.0
    for k, w in clips.items():
        one = StreamingTranscriber(m, dec, carry_context=True)
        t = one.feed_wave(pack([w]), [len(w)], final=True)
        want = np64(one.last_output[0][0, :one.last_output[1][0]])
        g = np64(torch.cat(got[k]))
        assert g.shape == want.shape, k
        worst = max(worst, float(np.abs(g - want).max()))
        if k in ("a", "c"):
            assert text[["a", "c"].index(k)] == t[0]
    print("pool feed_wave vs single-stream session: %.2e" % worst)
    assert worst <= 1e-4


def test_pool_in_lock_step_equals_the_session(model_case):
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.streaming import StreamPool
    fx, m, wavs = model_case[:3]
    got, per_feed, st = wave_session(m, fx, wavs, 3200)
    pool = StreamPool(m, D.GreedyDecoder(fx.labels), 2)
    sl = [pool.open(), pool.open()]
    pos, mine = 0, [[], []]
    for k in range(len(per_feed)):
        final = k == len(per_feed) - 1
        counts = [n - pos for n in WAVE_LENS] if final else [3200, 3200]
        text = pool.feed_wave(sl, pack([w[pos:pos + c] for w, c in zip(wavs, counts)]), counts, final=sl if final else ())
        pos += 3200
        for n in range(2):
            if sl[n] in pool.last_output:
                mine[n].append(pool.last_output[sl[n]])
    for n in range(2):
        assert torch.equal(torch.cat(mine[n]), torch.cat(got[n]))
    assert text == st.best()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(model_case):
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.streaming import StreamPool, StreamingTranscriber
    fx, m, wavs, spect = model_case[:4]
    dec = D.GreedyDecoder(fx.labels)
    with pytest.raises(ValueError, match="reflect"):
        front_end(pad_mode="reflect").stream(1, DEV)
    with pytest.raises(ValueError, match="not causal"):
        front_end(True).stream(1, DEV)
    w = pack([wavs[0][:3200], wavs[1][:3200]])
    with pytest.raises(ValueError, match="normalize=True"):
        StreamingTranscriber(m, dec, front_end=front_end(True), carry_context=True).feed_wave(w, [3200, 3200])
    st = StreamingTranscriber(m, dec, carry_context=True)
    with pytest.raises(ValueError, match="same sample count"):
        st.feed_wave(w, [3200, 3100])
    with pytest.raises(ValueError, match="descend"):
        st.feed_wave(w, [3100, 3200], final=True)
    assert st.feed_wave(w[:, :100].contiguous(), [100, 100]) == ['', ''] and st.last_output is None      # buffers only
    with pytest.raises(ValueError, match="feed_wave"):
        st.feed(spect[:, :, :, :20].contiguous(), [20, 20])
    st.end()
    assert st.frames == [1, 1]                                        # 100 samples: one frame, flushed by end()
    with pytest.raises(ValueError, match="ended"):
        st.feed_wave(w, [3200, 3200])
    st.reset()
    st.feed(spect[:, :, :, :20].contiguous(), [20, 20])              # after reset() either kind of feed may start
    with pytest.raises(ValueError, match="spectrogram chunks"):
        st.feed_wave(w, [3200, 3200])
    pool = StreamPool(m, dec, 2)
    a, b = pool.open(), pool.open()
    pool.feed_wave([a], w[:1], [3200])
    pool.feed([b], spect[:1, :, :, :20].contiguous(), [20])
    with pytest.raises(ValueError, match="feed_wave"):
        pool.feed([a], spect[:1, :, :, :20].contiguous(), [20])
    with pytest.raises(ValueError, match="spectrogram chunks"):
        pool.feed_wave([b], w[:1], [3200])
    pool.end([a, b])                                                  # one of each kind
    with pytest.raises(ValueError, match="ended"):
        pool.feed_wave([a], w[:1], [3200])
    pool.close(b)
    assert pool.open() == b
    pool.feed_wave([b], w[:1], [3200])                               # a reopened slot takes either kind again


# ---- 9. guard bytes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows,counts", [(1, [801]), (3, [2037, 100, 479]), (2, [0, 0])])
def test_stream_feed_stays_inside_out_the_workspace_and_the_state(n_rows, counts):
    """two feeds (the second final) through the raw ABI on byte buffers that are 4096 patterned bytes longer than the size
    queries say: the bytes behind out, the workspace and the state are as they were, and the frames are the handle's."""
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd._lib import call, query
    from deepspeech.pytorch_amd.spectrogram import plan_wave
    fe = front_end()
    S = n_rows + 1
    wavs = [clip(900 + k, 2 * n + 1) for k, n in enumerate(counts)]
    need_state = query("ds2_spect_stream_state_bytes", S)
    state = torch.full((need_state + 4096,), PATTERN, dtype=torch.uint8, device=DEV)
    handle = fe.stream(S, DEV)
    done = [0] * n_rows
    for final in (False, True):
        cnt = [len(w) - d for w, d in zip(wavs, done)] if final else counts
        chunk = pack([w[d:d + c] for w, d, c in zip(wavs, done, cnt)], max(max(cnt), 1))
        plans = [plan_wave(d, c, final) for d, c in zip(done, cnt)]
        Tc, mx = max(p.emit for p in plans), max(cnt)
        table = torch.tensor([(r + 1, r, 0 if not final else p.carried, c, p.frames_before, p.emit, int(final), int(not final))
                              for r, (c, p) in enumerate(zip(cnt, plans))], dtype=torch.int32, device=DEV)
        need_out, need_ws = n_rows * NBIN * Tc * 4, query("ds2_spect_stream_ws_bytes", n_rows, mx, Tc)
        out = torch.full((need_out + 4096,), PATTERN, dtype=torch.uint8, device=DEV)
        ws = torch.full((need_ws + 4096,), PATTERN, dtype=torch.uint8, device=DEV)
        call("ds2_spect_stream_feed", ops.P(chunk), chunk.stride(0), ops.P(table), n_rows, mx, Tc, S, ops.P(fe._basis_on(chunk.device)), 2,
             fe.running_floor, *fe.running_prior, ops.P(state), ops.P(out), ops.P(ws), ops.S())
        torch.cuda.synchronize()
        want, frames = handle.feed(range(1, S), chunk, cnt, final=range(1, S) if final else ())
        assert frames == [p.emit for p in plans]
        assert torch.equal(out[:need_out].view(torch.float32).view(n_rows, 1, NBIN, Tc), want)
        assert bool((out[need_out:] == PATTERN).all()) and bool((ws[need_ws:] == PATTERN).all())
        assert bool((state[need_state:] == PATTERN).all())
        assert bool((state[:16] == PATTERN).all()) and bool((state[16 * S:16 * S + 1280] == PATTERN).all())   # slot 0 is not in the table
        done = [d + c for d, c in zip(done, cnt)]


@pytest.mark.parametrize("N,Lmax", [(1, 159), (3, 801), (2, 10240)])
def test_running_call_stays_inside_out_and_the_workspace(N, Lmax):
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd._lib import call, query
    lens = [Lmax, max(1, Lmax // 2), 2][:N]
    fe = front_end()
    wav = pack([clip(600 + k, n) for k, n in enumerate(lens)])
    ref = fe(wav, lens)[0]
    Tmax = 1 + Lmax // HOP
    need_out, need_ws = N * NBIN * Tmax * 4, query("ds2_spect_running_ws_bytes", N, Lmax)
    out = torch.full((need_out + 4096,), PATTERN, dtype=torch.uint8, device=DEV)
    ws = torch.full((need_ws + 4096,), PATTERN, dtype=torch.uint8, device=DEV)
    ns = torch.tensor(lens, dtype=torch.int32, device=DEV)
    null = ops.P(None)
    call("ds2_spectrogram_running", ops.P(wav), wav.stride(0), ops.P(ns), N, Lmax, ops.P(fe._basis_on(wav.device)), 0, fe.running_floor,
         *fe.running_prior, ops.P(out), ops.P(ws), 0, null, 0, null, 0, null, 0, null, ops.S())
    torch.cuda.synchronize()
    assert torch.equal(out[:need_out].view(torch.float32).view(N, 1, NBIN, Tmax), ref) and torch.isfinite(ref).all()
    assert bool((out[need_out:] == PATTERN).all()) and bool((ws[need_ws:] == PATTERN).all())
