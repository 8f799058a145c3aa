"""GPU checks of the resampler (csrc/ds2_resample.hip: k_resample, k_resample_stream,
k_resample_stream_carry; resample.Resampler / ResampleStream, SpectrogramFrontEnd(input_rate=...), SpectStream, feed_wave).

The oracle is the definition restated in numpy (tests/resample_reference.py).  With integer taps and integer samples every sum
stays below 2^24 (|h| <= 8, |x| <= 64, 2W <= 144 taps: 73728), so any order of the fp32 sum is exact and the device must give the
oracle's integers: torch.equal.  With the real taps the bound is the standard one for a sum of 2W products in any order,
(2W + 1) 2^-24 sum_j |h32[p][j] x|, computed from the oracle's own operands (the fp32-rounded taps, in fp64).  Everything between
the streaming form and the one-shot call is torch.equal: the order of a sample's sum depends on the tap index alone."""
import numpy as np
import pytest
import torch

import resample_reference as RR
from fixtures import DEV, Fixture, np64
from test_gpu_model import build

pytestmark = pytest.mark.gpu
HOP, NBIN = 160, 161
SHAPES = [(2, 1, 24), (1, 3, 72), (160, 441, 67), (640, 441, 24)]
UNSTAGED = (1, 200, 4800)          # 3.2 MHz: 2W + D / U samples exceed the LDS span, the kernels read the input from global memory
GARBAGE = 77.0


def tile_of(U, D, W):
    from deepspeech.pytorch_amd._lib import query
    return query("ds2_resample_tile", U, D, W)


def device_resample(clips, taps, U, D, W, pad=13):
    """clips: 1-D float arrays -> (out (N, max out_len) on the device, nsamples_out).  The buffer is `pad` samples wider than the
    longest clip and holds non-zero garbage beyond every clip's own samples."""
    from deepspeech.pytorch_amd import ops
    lens = [len(c) for c in clips]
    buf = torch.full((len(clips), max(lens) + pad), GARBAGE)
    for i, c in enumerate(clips):
        buf[i, :len(c)] = torch.from_numpy(np.asarray(c, dtype=np.float32))
    ldo = max(RR.out_len(n, U, D) for n in lens)
    return ops.resample(buf.to(DEV), lens, torch.from_numpy(np.asarray(taps, dtype=np.float32)).to(DEV), U, D, W, ldo)


def inputs_for(outputs, U, D):
    """the shortest clip with at least `outputs` output samples"""
    n = (outputs * D) // U
    while RR.out_len(n, U, D) < outputs:
        n += 1
    return n


# ---- 1. integer operands, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,D,W", SHAPES + [UNSTAGED])
def test_integer_operands_equal_the_oracle_bit_for_bit(U, D, W):
    """ragged batches of 3: lengths 1, W, W + 1, 2W, and clips that end one output short of, on and one past the seam behind the
    kernel's second tile (three tiles) and around the first (where U > D every output count is a multiple of U / D: the nearest).  The last
    shape has 9600 taps: |sum| <= 9600 * 8 * 64 < 2^24 still."""
    T = tile_of(U, D, W)
    h = RR.integer_taps(U, W)
    rng = np.random.RandomState(U + D)
    batches = [[inputs_for(2 * T + 1, U, D), 2 * W, 1], [inputs_for(2 * T, U, D), W + 1, W],
               [inputs_for(2 * T - 1, U, D), inputs_for(T + 1, U, D), inputs_for(T, U, D)]]
    assert RR.out_len(batches[0][0], U, D) > 2 * T                      # three tiles
    for lens in batches:
        clips = [rng.randint(-64, 65, size=n).astype(np.int64) for n in lens]
        out, ns_out = device_resample(clips, h, U, D, W)
        assert ns_out.tolist() == [RR.out_len(n, U, D) for n in lens]
        for i, c in enumerate(clips):
            want = RR.resample(c, h, U, D, W)
            assert np.abs(want).max() < 2 ** 24
            assert torch.equal(out[i, :len(want)].cpu(), torch.from_numpy(want.astype(np.float32))), (lens, i)
            assert not out[i, len(want):].any()                        # zero beyond the clip's outputs: no garbage leaks in


@pytest.mark.parametrize("U,D,W", SHAPES)
def test_an_impulse_at_every_position_pins_every_phase_and_tap(U, D, W):
    """one clip of D + 2W samples per impulse position, all in one launch: output m shows taps[p(m)][i - n0(m) + W - 1] * 64 and
    nothing else, and over a full period of D inputs every (phase, tap) pair appears"""
    L = D + 2 * W
    h = RR.integer_taps(U, W)
    clips = 64 * np.eye(L, dtype=np.int64)
    out, _ = device_resample(list(clips), h, U, D, W)
    M = RR.out_len(L, U, D)
    m = np.arange(M, dtype=np.int64)
    n0, p = (m * D) // U, (m * D) % U
    j = np.arange(L)[:, None] - n0[None, :] + W - 1                     # [position][output]
    want = np.where((j >= 0) & (j < 2 * W), 64 * h[p[None, :], np.clip(j, 0, 2 * W - 1)], 0)
    seen = np.zeros((U, 2 * W), bool)
    ok = (j >= 0) & (j < 2 * W)
    seen[np.broadcast_to(p[None, :], j.shape)[ok], j[ok]] = True
    assert seen.all()
    assert torch.equal(out[:, :M].cpu(), torch.from_numpy(want.astype(np.float32)))


def test_indices_beyond_2_to_the_31():
    """one 44100 Hz clip of 13.7 M samples (310 s): m D passes 2^31 at output 4.87 M.  The last 4096 outputs and 4096 random ones
    against the integer oracle."""
    from deepspeech.pytorch_amd import ops
    U, D, W = 160, 441, 67
    n = 13_700_000
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randint(-64, 65, (1, n), device=DEV, generator=g).float()
    h = RR.integer_taps(U, W)
    M = RR.out_len(n, U, D)
    assert (M - 1) * D > 2 ** 31
    out, ns_out = ops.resample(x, [n], torch.from_numpy(h.astype(np.float32)).to(DEV), U, D, W, M)
    assert ns_out.tolist() == [M]
    ms = np.unique(np.concatenate([np.arange(M - 4096, M), np.random.RandomState(1).randint(0, M, 4096)]))
    assert (ms * D > 2 ** 31).sum() >= 4096
    want = RR.resample(x[0].cpu().numpy().astype(np.int64), h, U, D, W, ms=ms)
    got = out[0].cpu()[torch.from_numpy(ms)]
    assert torch.equal(got, torch.from_numpy(want.astype(np.float32)))


# ---- 2. the real taps against fp64 ---------------------------------------------------------------------------------------------
def sine(freq, rate, n, amp=1.0):
    return (amp * np.sin(2 * np.pi * freq * np.arange(n) / rate)).astype(np.float32)


@pytest.mark.parametrize("rate", RR.RATES)
def test_real_taps_stay_inside_the_summation_bound(rate):
    """random noise, a sine at a quarter of the lower Nyquist frequency and a short clip, ragged: per output
    |y - y64| <= (2W + 1) 2^-24 sum_j |h32[p][j] x|"""
    from deepspeech.pytorch_amd.resample import Resampler
    rs = Resampler(rate)
    U, D, W = rs.up, rs.down, rs.half_width
    n = 5 * D + 2 * W + 11
    rng = np.random.RandomState(rate)
    clips = [(0.3 * rng.standard_normal(n)).astype(np.float32), sine(min(rate, 16000) / 8.0, rate, n - 37, 0.8),
             (0.3 * rng.standard_normal(W + 3)).astype(np.float32)]
    buf = torch.zeros((3, n))
    for i, c in enumerate(clips):
        buf[i, :len(c)] = torch.from_numpy(c)
    out, ns16 = rs(buf.to(DEV), [len(c) for c in clips])
    assert ns16.tolist() == [rs.out_len(len(c)) for c in clips] and out.shape[1] == rs.out_len(n)
    h = rs.taps.astype(np.float64)
    worst = 0.0
    for i, c in enumerate(clips):
        want = RR.resample(c.astype(np.float64), h, U, D, W)
        allowed = (2 * W + 1) * 2.0 ** -24 * RR.resample(c.astype(np.float64), h, U, D, W, magnitude=True)
        err = np.abs(np64(out[i, :len(want)]) - want)
        worst = max(worst, float((err / np.maximum(allowed, 1e-30)).max()))
        assert (err <= allowed).all(), (rate, i, float(err.max()))
        assert not out[i, len(want):].any()
    print("%d Hz: worst |y - y64| / bound = %.3f" % (rate, worst))


def test_a_sine_in_the_passband_keeps_its_amplitude_and_one_above_nyquist_is_removed():
    """48000 Hz: 1 kHz comes out as the same sine at 16 kHz (the filter has no delay), within 0.1 % of the amplitude in the
    interior; 10 kHz, above the new Nyquist frequency, comes out below 1e-4 of its amplitude"""
    from deepspeech.pytorch_amd.resample import Resampler
    rs = Resampler(48000)
    n = 9600
    buf = torch.from_numpy(np.stack([sine(1000, 48000, n), sine(10000, 48000, n)])).to(DEV)
    out, ns16 = rs(buf, [n, n])
    assert ns16.tolist() == [3200, 3200]
    y = np64(out)[:, 100:-100]
    m = np.arange(100, 3100)
    print("1 kHz: max |y - sin| %.2e, 10 kHz: max |y| %.2e" % (np.abs(y[0] - np.sin(2 * np.pi * m / 16.0)).max(), np.abs(y[1]).max()))
    assert np.abs(y[0] - np.sin(2 * np.pi * m / 16.0)).max() <= 1e-3 and abs(np.abs(y[0]).max() - 1.0) <= 1e-3
    assert np.abs(y[1]).max() <= 1e-4


# ---- 3. streaming == one-shot, bit for bit -------------------------------------------------------------------------------------
def clip(seed, n, scale=0.1):
    return (np.random.RandomState(seed).standard_normal(n) * scale).astype(np.float32)


def pack(wavs, width=None):
    buf = torch.zeros((len(wavs), width if width is not None else max(len(w) for w in wavs)))
    for i, w in enumerate(wavs):
        buf[i, :len(w)] = torch.from_numpy(w)
    return buf.to(DEV)


_ONE_SHOT = {}


def one_shot(rate, lens, seed):
    """the clips and their one-shot resampled batch, computed once"""
    from deepspeech.pytorch_amd.resample import Resampler
    key = (rate, tuple(lens), seed)
    if key not in _ONE_SHOT:
        wavs = [clip(seed + 7 * k + n, n) for k, n in enumerate(lens)]
        rs = Resampler(rate)
        out, ns16 = rs(pack(wavs), lens)
        _ONE_SHOT[key] = (rs, wavs, out.clone(), ns16.tolist())
    return _ONE_SHOT[key]


def run_streams(st, slots, wavs, per_row, seed, empty_every=3):
    """Feeds row r of `wavs` (slot slots[r]) per_row[r] samples a tick (None: the whole clip) until it ends, the row whose clip is
    used up with final; the rows of a tick in shuffled order, an empty feed of every running row in front of every third tick.
    Returns per row the concatenated output."""
    rng = np.random.RandomState(seed)
    pos, got, live, tick = [0] * len(wavs), [[] for _ in wavs], list(range(len(wavs))), 0
    while live:
        if tick % empty_every == 0:
            out, counts = st.feed([slots[r] for r in live], torch.zeros((len(live), 0), device=DEV), [0] * len(live))
            for r, c, o in zip(live, counts, out):
                got[r].append(o[:c])
        rows = [live[i] for i in rng.permutation(len(live))]
        counts = [len(wavs[r]) - pos[r] if per_row[r] is None else min(per_row[r], len(wavs[r]) - pos[r]) for r in rows]
        final = [r for r, c in zip(rows, counts) if pos[r] + c == len(wavs[r])]
        chunk = pack([wavs[r][pos[r]:pos[r] + c] for r, c in zip(rows, counts)], max(counts) + 3)
        out, emitted = st.feed([slots[r] for r in rows], chunk, counts, final=[slots[r] for r in final])
        assert tuple(out.shape) == (len(rows), max(emitted))
        for r, c, e, o in zip(rows, counts, emitted, out):
            assert not o[e:].any()
            got[r].append(o[:e])
            pos[r] += c
        live = [r for r in live if r not in final]
        tick += 1
    return [torch.cat(g) for g in got]


@pytest.mark.parametrize("feed", ["1", "W-1", "W", "W+1", "2W", "97", "whole"])
@pytest.mark.parametrize("rate", [8000, 11025, 44100, 48000])
def test_streaming_equals_the_one_shot_call(rate, feed):
    """four clips of 6W + 5, 3W + 2, W + 1 and 1 samples on slots 3, 0, 2, 1 of five; row r brings the feed size + r samples a
    tick, so the rows differ; slot 4 is never fed"""
    U, D, W = RR.params(rate)
    lens = [6 * W + 5, 3 * W + 2, W + 1, 1]
    rs, wavs, ref, ns16 = one_shot(rate, lens, 100)
    c = {"1": 1, "W-1": W - 1, "W": W, "W+1": W + 1, "2W": 2 * W, "97": 97, "whole": None}[feed]
    st = rs.stream(5, DEV)
    got = run_streams(st, [3, 0, 2, 1], wavs, [None if c is None else c + r for r in range(4)], seed=rate + (c or 0))
    for r, n16 in enumerate(ns16):
        assert got[r].shape[0] == n16 and torch.equal(got[r], ref[r, :n16]), (rate, feed, r)
    assert st.samples == [lens[1], lens[3], lens[2], lens[0], 0] and st.ended == [True] * 4 + [False]


@pytest.mark.parametrize("feed", ["2W", "whole"])
def test_streaming_equals_the_one_shot_call_on_the_path_without_a_staged_span(feed):
    rate = 16000 * UNSTAGED[1]
    U, D, W = RR.params(rate)
    assert (U, D, W) == UNSTAGED
    lens = [6 * W + 5, 3 * W + 2, W + 1, 1]
    rs, wavs, ref, ns16 = one_shot(rate, lens, 700)
    st = rs.stream(4, DEV)
    got = run_streams(st, [3, 0, 2, 1], wavs, [None if feed == "whole" else 2 * W + r for r in range(4)], seed=9)
    for r, n16 in enumerate(ns16):
        assert got[r].shape[0] == n16 and torch.equal(got[r], ref[r, :n16]), (feed, r)
    want = RR.resample(wavs[1].astype(np.float64), rs.taps.astype(np.float64), U, D, W)
    bound = (2 * W + 1) * 2.0 ** -24 * RR.resample(wavs[1].astype(np.float64), rs.taps.astype(np.float64), U, D, W, magnitude=True)
    assert (np.abs(np64(ref[1, :ns16[1]]) - want) <= bound).all()


@pytest.mark.parametrize("rate", [8000, 44100])
def test_a_reused_slot_starts_fresh_and_untouched_slots_keep_their_state(rate):
    U, D, W = RR.params(rate)
    lens = [6 * W + 5, 4 * W + 1]
    rs, wavs, ref, ns16 = one_shot(rate, lens, 300)
    st = rs.stream(4, DEV)
    loud = clip(1, 5 * W, 0.7) + 0.3
    st.feed([0, 1, 3], pack([loud, loud, loud]), [2 * W + 3, 3 * W, 5 * W])              # three slots left mid-utterance
    state = lambda: st._state.view(torch.float32).view(4, 2 * W).clone()
    before = state()
    assert before[[0, 1, 3]].any(1).all() and not before[2].any()
    st.reset([1])
    assert torch.equal(state(), before)                                                  # reset launches nothing
    got = [[], []]
    a, e = st.feed([1], pack([wavs[0][:7]]), [7])                                        # slot 1 reused while 0 and 3 run
    got[0].append(a[0, :e[0]])
    after = state()
    assert torch.equal(after[[0, 2, 3]], before[[0, 2, 3]])                              # the others, bit for bit
    assert torch.equal(after[1, :7].cpu(), torch.from_numpy(wavs[0][:7]))
    a, e = st.feed([2, 1], pack([wavs[1][:3 * W], wavs[0][7:7 + 2 * W]]), [3 * W, 2 * W])
    got[1].append(a[0, :e[0]])
    got[0].append(a[1, :e[1]])
    assert torch.equal(state()[[0, 3]], before[[0, 3]])
    a, e = st.feed([1, 2], pack([wavs[0][7 + 2 * W:], wavs[1][3 * W:]]), [lens[0] - 7 - 2 * W, lens[1] - 3 * W], final=[1, 2])
    got[0].append(a[0, :e[0]])
    got[1].append(a[1, :e[1]])
    for r in range(2):
        assert torch.equal(torch.cat(got[r]), ref[r, :ns16[r]])
    with pytest.raises(ValueError, match="ended"):
        st.feed([1], torch.zeros((1, 4), device=DEV), [4])
    st.reset()                                                                           # all slots; 0 and 3 were mid-utterance
    out = run_streams(st, [0, 3], wavs, [97, None], seed=3)
    assert torch.equal(out[0], ref[0, :ns16[0]]) and torch.equal(out[1], ref[1, :ns16[1]])


def test_a_final_feed_of_nothing_flushes_the_tail():
    rs, wavs, ref, ns16 = one_shot(44100, [4410, 1000], 500)
    st = rs.stream(2, DEV)
    a, e = st.feed([0, 1], pack(wavs), [4410, 1000])
    b, f = st.feed([1, 0], torch.zeros((2, 0), device=DEV), [0, 0], final=[0, 1])
    assert [e[0] + f[1], e[1] + f[0]] == ns16 and min(f) > 0
    assert torch.equal(torch.cat([a[0, :e[0]], b[1, :f[1]]]), ref[0, :ns16[0]])
    assert torch.equal(torch.cat([a[1, :e[1]], b[0, :f[0]]]), ref[1, :ns16[1]])


# ---- 4. the front-end ----------------------------------------------------------------------------------------------------------
def front_end(normalize="running", **kw):
    from deepspeech.pytorch_amd import configs
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    return SpectrogramFrontEnd(configs.SpectConfig(), normalize=normalize, **kw)


@pytest.mark.parametrize("normalize", [True, False, "running"])
@pytest.mark.parametrize("rate", [8000, 44100])
def test_front_end_with_input_rate_equals_resampler_then_front_end(rate, normalize):
    from deepspeech.pytorch_amd.resample import Resampler
    lens = [9000, 4410, 300]
    wav = pack([clip(40 + k, n) for k, n in enumerate(lens)], 9100)
    got, pct, frames = front_end(normalize, input_rate=rate)(wav, lens)
    rs = Resampler(rate)
    wav16, ns16 = rs(wav, lens)
    want, pct16, frames16 = front_end(normalize)(wav16, ns16)
    assert torch.equal(got, want) and torch.equal(pct, pct16) and torch.equal(frames, frames16)
    assert frames.tolist() == [1 + rs.out_len(n) // HOP for n in lens] and got.shape[3] == frames.max()


def test_sixteen_khz_input_rate_is_what_none_is():
    lens = [5000, 801]
    wav = pack([clip(60 + k, n) for k, n in enumerate(lens)])
    fe = front_end(input_rate=16000)
    assert fe.resampler is None and front_end(input_rate=None).resampler is None
    a, b = fe(wav, lens), front_end()(wav, lens)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    st = fe.stream(2, DEV)
    assert st._resample is None
    s1, f1 = st.feed([0, 1], wav, lens, final=[0, 1])
    s2, f2 = front_end().stream(2, DEV).feed([0, 1], wav, lens, final=[0, 1])
    assert torch.equal(s1, s2) and f1 == f2


def test_front_end_stream_at_44100_equals_the_one_shot_running_call():
    """chunks of 441, 4410 and 1000 samples at 44100 Hz in turn; ``samples`` and ``frames`` count the 16 kHz signal"""
    lens = [30000, 21000]
    wavs = [clip(70 + k, n) for k, n in enumerate(lens)]
    fe = front_end(input_rate=44100)
    ref, _, frames = fe(pack(wavs), lens)
    st = fe.stream(3, DEV)
    slots, pos, got, k, live = [2, 0], [0, 0], [[], []], 0, [0, 1]
    while live:
        c = (441, 4410, 1000)[k % 3]
        counts = [min(c, lens[r] - pos[r]) for r in live]
        final = [r for r, n in zip(live, counts) if pos[r] + n == lens[r]]
        out, fr = st.feed([slots[r] for r in live], pack([wavs[r][pos[r]:pos[r] + n] for r, n in zip(live, counts)]), counts,
                          final=[slots[r] for r in final])
        for i, r in enumerate(live):
            got[r].append(out[i, 0, :, :fr[i]])
            pos[r] += counts[i]
        live, k = [r for r in live if r not in final], k + 1
    for r in range(2):
        assert st.frames(slots[r]) == frames[r] and st.samples[slots[r]] == fe.resampler.out_len(lens[r])
        assert torch.equal(torch.cat(got[r], 1), ref[r, 0, :, :frames[r]])
    st.reset()
    assert st.samples == [0, 0, 0] and st._resample.samples == [0, 0, 0]


def test_collate_and_wave_augment_follow_the_resampled_lengths():
    from deepspeech.pytorch_amd.augment import WaveAugment
    from deepspeech.pytorch_amd.resample import Resampler
    rate = 44100
    waves = [torch.from_numpy(clip(80 + k, n)) for k, n in enumerate((11025, 24000, 1323))]
    fe = front_end(input_rate=rate)
    inputs, pct, order = fe.collate(waves)
    assert order == [1, 0, 2] == front_end().collate(waves)[2]
    lens = [len(waves[i]) for i in order]
    want, want_pct, frames = fe(pack([waves[i].numpy() for i in order]), lens)
    assert torch.equal(inputs, want) and torch.equal(pct, want_pct)
    assert frames.tolist() == [1 + fe.resampler.out_len(n) // HOP for n in lens]
    assert pct.tolist() == [np.float32(f / float(frames.max())) for f in frames.tolist()]
    # waveform augmentation sees the 16 kHz signal: the same draws as a 16 kHz front-end handed the resampled clips
    wa = WaveAugment(speed_volume_perturb=True)
    batch, ns = pack([w.numpy() for w in waves]), [len(w) for w in waves]
    got = front_end(wave_augment=wa, rng=np.random.default_rng(2), input_rate=rate)(batch, ns)
    ref = front_end(wave_augment=wa, rng=np.random.default_rng(2))(*Resampler(rate)(batch, ns))
    assert all(torch.equal(x, y) for x, y in zip(got, ref))
    a = front_end(wave_augment=wa, rng=np.random.default_rng(3), input_rate=rate).collate(waves)
    fe16 = front_end(wave_augment=wa, rng=np.random.default_rng(3))
    wav16, ns16 = Resampler(rate)(batch, ns)
    b = fe16.collate([wav16[i, :n].cpu() for i, n in enumerate(ns16.tolist())])
    assert a[2] == b[2] and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 5. sessions ---------------------------------------------------------------------------------------------------------------
RATE = 44100
SESSION_LENS = [33075, 30000, 26460]


@pytest.fixture(scope="module")
def session_case():
    """gru_uni_la's weights, three 44100 Hz clips and their one-shot 16 kHz versions on the host"""
    from deepspeech.pytorch_amd.resample import Resampler
    fx = Fixture("gru_uni_la")
    m = build(fx, 32).eval()
    rng = np.random.RandomState(17)
    wavs = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in SESSION_LENS]
    rs = Resampler(RATE)
    out, ns16 = rs(pack(wavs), SESSION_LENS)
    wavs16 = [out[i, :n].cpu().numpy() for i, n in enumerate(ns16.tolist())]
    return fx, m, rs, wavs, wavs16


def test_pool_fed_44100_hz_chunks_equals_the_pool_fed_the_resampled_audio(session_case):
    """three streams that join one tick apart, 4410 samples (0.1 s) a tick.  The reference pool gets the one-shot-resampled clips
    in the chunks the resampler's plan says each feed emits, so both pools complete the same frames in every feed: the same
    transcripts after every feed and the same probabilities, torch.equal"""
    from deepspeech.pytorch_amd import decoder as Dc
    from deepspeech.pytorch_amd.streaming import StreamPool
    fx, m, rs, wavs, wavs16 = session_case
    dec = Dc.GreedyDecoder(fx.labels)
    pool, ref = StreamPool(m, dec, 3, front_end=front_end(input_rate=RATE)), StreamPool(m, dec, 3, front_end=front_end())
    slot, pos, pos16, got, want, done, tick = {}, {}, {}, {r: [] for r in range(3)}, {r: [] for r in range(3)}, set(), 0
    while len(done) < 3:
        if tick < 3:
            slot[tick] = pool.open()
            assert ref.open() == slot[tick]
            pos[tick] = pos16[tick] = 0
        rows = [r for r in slot if r not in done]
        counts = [min(4410, len(wavs[r]) - pos[r]) for r in rows]
        final = [r for r, c in zip(rows, counts) if pos[r] + c == len(wavs[r])]
        plans = [rs.plan_resample(pos[r], c, r in final) for r, c in zip(rows, counts)]
        assert all(p.out_before == pos16[r] for r, p in zip(rows, plans))
        t1 = pool.feed_wave([slot[r] for r in rows], pack([wavs[r][pos[r]:pos[r] + c] for r, c in zip(rows, counts)]), counts,
                            final=[slot[r] for r in final])
        t2 = ref.feed_wave([slot[r] for r in rows], pack([wavs16[r][pos16[r]:pos16[r] + p.emit] for r, p in zip(rows, plans)]),
                           [p.emit for p in plans], final=[slot[r] for r in final])
        assert t1 == t2, tick
        assert set(pool.last_output) == set(ref.last_output)
        for r, c, p in zip(rows, counts, plans):
            if slot[r] in pool.last_output:
                got[r].append(pool.last_output[slot[r]])
                want[r].append(ref.last_output[slot[r]])
            pos[r], pos16[r] = pos[r] + c, pos16[r] + p.emit
        done |= set(final)
        tick += 1
    for r in range(3):
        assert pos16[r] == len(wavs16[r]) and torch.cat(got[r]).shape[0] > 0
        assert torch.equal(torch.cat(got[r]), torch.cat(want[r]))


def test_transcriber_fed_44100_hz_chunks_equals_the_one_fed_the_resampled_audio(session_case):
    from deepspeech.pytorch_amd import decoder as Dc
    from deepspeech.pytorch_amd.streaming import StreamingTranscriber
    fx, m, rs, wavs, wavs16 = session_case
    dec = Dc.GreedyDecoder(fx.labels)
    st = StreamingTranscriber(m, dec, front_end=front_end(input_rate=RATE), carry_context=True)
    ref = StreamingTranscriber(m, dec, front_end=front_end(), carry_context=True)
    pos = pos16 = 0
    got, want = [[], [], []], [[], [], []]
    while True:
        final = min(SESSION_LENS) - pos <= 4410
        counts = [n - pos for n in SESSION_LENS] if final else [4410] * 3
        emits = [rs.plan_resample(pos, c, final).emit for c in counts]
        t1 = st.feed_wave(pack([w[pos:pos + c] for w, c in zip(wavs, counts)]), counts, final=final)
        t2 = ref.feed_wave(pack([w[pos16:pos16 + e] for w, e in zip(wavs16, emits)]), emits, final=final)
        assert t1 == t2 and (st.last_output is None) == (ref.last_output is None)
        if st.last_output is not None:
            for n in range(3):
                got[n].append(st.last_output[0][n, :st.last_output[1][n]])
                want[n].append(ref.last_output[0][n, :ref.last_output[1][n]])
        pos, pos16 = pos + 4410, pos16 + emits[0]
        if final:
            break
    for n in range(3):
        assert torch.equal(torch.cat(got[n]), torch.cat(want[n]))
    assert st.frames == ref.frames and st.best() == ref.best()


# ---- 6. refusals and guard bytes -----------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_nothing_is_written():
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd._lib import Ds2HipError
    from deepspeech.pytorch_amd.resample import Resampler
    rs = Resampler(8000)
    wav = pack([clip(1, 100)])
    out = torch.full((1, 200), GARBAGE, device=DEV)
    taps = rs.taps_on(wav.device)
    for U, D, W in ((0, 1, 24), (2, 0, 24), (2, 1, 0), (16384, 1, 24)):
        with pytest.raises(Ds2HipError, match="1002"):
            ops.resample(wav, [100], taps, U, D, W, 200, out=out)
    torch.cuda.synchronize()
    assert bool((out == GARBAGE).all())
    with pytest.raises(Ds2HipError, match="no CPU path"):
        rs(wav.cpu(), [100])
    with pytest.raises(ValueError, match="positive sample count"):
        rs(wav, [0])
    with pytest.raises(ValueError, match="exceeds"):
        rs(wav, [101])


@pytest.mark.parametrize("rate,counts", [(8000, [801, 3]), (44100, [2037, 100]), (48000, [0, 0])])
def test_stream_feed_stays_inside_out_the_workspace_and_the_state(rate, counts):
    """two feeds (the second final) through the raw ABI on buffers that are 1024 patterned floats longer than the size queries
    say: the floats behind out, the workspace and the state are as they were, and so is the slot that is not in the table"""
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd._lib import call, query
    from deepspeech.pytorch_amd.resample import Resampler
    rs = Resampler(rate)
    U, D, W = rs.up, rs.down, rs.half_width
    S = 3
    wavs = [clip(900 + k, 2 * n + 1) for k, n in enumerate(counts)]
    need_state = query("ds2_resample_stream_state_bytes", S, W) // 4
    state = torch.full((need_state + 1024,), GARBAGE, device=DEV)
    handle = rs.stream(S, DEV)
    done = [0, 0]
    for final in (False, True):
        cnt = [len(w) - d for w, d in zip(wavs, done)] if final else counts
        chunk = pack([w[d:d + c] for w, d, c in zip(wavs, done, cnt)], max(max(cnt), 1))
        plans = [rs.plan_resample(d, c, final) for d, c in zip(done, cnt)]
        me, mx = max(p.emit for p in plans), max(cnt)
        table = np.zeros((2, 10), np.int32)
        for r, (c, p) in enumerate(zip(cnt, plans)):
            table[r] = (r + 1, r, p.carried, c, p.out_before, 0, p.emit, int(final), int(not final), 0)
        table = torch.from_numpy(table).to(DEV)
        need_ws = query("ds2_resample_stream_ws_bytes", 2, W) // 4
        out = torch.full((2 * me + 1024,), GARBAGE, device=DEV)
        ws = torch.full((need_ws + 1024,), GARBAGE, device=DEV)
        call("ds2_resample_stream_feed", ops.P(chunk), chunk.stride(0), ops.P(table), 2, mx, me, S, ops.P(rs.taps_on(chunk.device)), U, D, W,
             ops.P(state), ops.P(out) if me else ops.P(None), me, ops.P(ws), ops.S())
        torch.cuda.synchronize()
        want, emitted = handle.feed([1, 2], chunk, cnt, final=[1, 2] if final else ())
        assert emitted == [p.emit for p in plans]
        assert torch.equal(out[:2 * me].view(2, me), want)
        assert bool((out[2 * me:] == GARBAGE).all()) and bool((ws[need_ws:] == GARBAGE).all())
        assert bool((state[need_state:] == GARBAGE).all()) and bool((state[:2 * W] == GARBAGE).all())
        done = [d + c for d, c in zip(done, cnt)]
