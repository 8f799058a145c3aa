"""GPU checks of the reverberation kernel (csrc/ds2_reverb.hip, ops.reverb) and of SpectrogramFrontEnd with
WaveAugment(rir_bank=...) against the fp64 / int64 restatement tests/reverb_reference.py.

Integers: x in [-8, 8], h in [-4, 4], so every partial sum is at most 32 K <= 2^19 in magnitude for K <= 16384 and any fp32 order
is exact: the output equals the int64 convolution bit for bit.  Floats: |out - ref64| <= 2 K 2^-24 sum_k |h[k]| |x[i + p - k]|, the
gamma_K bound of a K-term chain of fp32 fused multiply-adds in any order, doubled for the final rounding of the comparison."""
import numpy as np
import pytest
import torch

import reverb_reference as R

pytestmark = pytest.mark.gpu

FILL = 7.0                                                  # what the output buffers hold before the kernel runs
KS = (1, 2, 31, 32, 33, 63, 64, 65, 1000)
ERR_ARG = 1002


def ops():
    from deepspeech.pytorch_amd import ops as o
    return o


def tile():
    from deepspeech.pytorch_amd import _lib
    return _lib.query("ds2_reverb_tile")


def lengths():
    t = tile()
    return (1, 31, 32, 33, t - 1, t, t + 1, 3 * t + 17)


def peaks(K):
    return sorted({0, 1 if K > 1 else 0, K // 2, K - 1})


def seam_cases():
    """every (K, L, p) of the grid, in batches of up to 8 rows that mix them: rows of one batch have different K, L and p."""
    cases = [(K, L, p) for K in KS for L in lengths() for p in peaks(K)]
    order = np.random.default_rng(0).permutation(len(cases))
    cases = [cases[i] for i in order]
    return [cases[i:i + 8] for i in range(0, len(cases), 8)]


def run_batch(cases, make_x, make_h, pad=3, dry=()):
    """cases: (K, L, p) per row.  The bank holds a guard pattern before and after every response; out is the middle of a larger
    buffer filled with FILL.  Rows in `dry` get rir_off = -1.  Returns (xs, hs, out rows (N, ldo), ldo)."""
    o = ops()
    N = len(cases)
    ldw = max(L for _, L, _ in cases) + pad
    ldo = ldw + 5
    x = np.full((N, ldw), 0.25, np.float32)                 # beyond a clip the input is not zero: nothing may read it
    xs, hs, parts, off = [], [], [], []
    pos = 0
    for n, (K, L, p) in enumerate(cases):
        xs.append(make_x(L))
        hs.append(make_h(K))
        x[n, :L] = xs[-1]
        parts += [np.full(5, 1000.0, np.float32), hs[-1].astype(np.float32)]
        off.append(-1 if n in dry else pos + 5)
        pos += 5 + K
    parts.append(np.full(5, 1000.0, np.float32))
    bank = torch.from_numpy(np.concatenate(parts)).cuda()
    big = torch.full((N + 2, ldo), FILL, dtype=torch.float32, device="cuda")
    xd = torch.from_numpy(x).cuda()
    o.reverb(xd, [L for _, L, _ in cases], bank, np.array(off, np.int64), np.array([K for K, _, _ in cases], np.int32),
             np.array([p for _, _, p in cases], np.int32), out=big[1:N + 1])
    got = big.cpu().numpy()
    assert np.all(got[0] == FILL) and np.all(got[-1] == FILL)                # nothing outside the (N, ldo) region
    assert np.array_equal(xd.cpu().numpy(), x)                                # out of place
    return xs, hs, got[1:N + 1], ldo


def int_x(rng):
    return lambda L: rng.integers(-8, 9, L).astype(np.float32)


def int_h(rng):
    def make(K):
        h = rng.integers(-4, 5, K).astype(np.float32)
        h[0] = h[0] or 1.0
        h[-1] = h[-1] or -3.0                                                 # the first and the last tap count
        return h
    return make


# ---- 1. exact on integers ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def integer_batches():
    rng = np.random.default_rng(1)
    res = []
    for cases in seam_cases():
        xs, hs, out, ldo = run_batch(cases, int_x(rng), int_h(rng))
        res.append((cases, xs, hs, out, ldo))
    return res


def test_the_grid_is_complete(integer_batches):
    seen = {c for cases, *_ in integer_batches for c in cases}
    assert seen == {(K, L, p) for K in KS for L in lengths() for p in peaks(K)}
    assert all(len(cases) <= 8 for cases, *_ in integer_batches)
    assert any(len({K for K, _, _ in cases}) > 4 and len({L for _, L, _ in cases}) > 4 for cases, *_ in integer_batches)


def test_integer_batches_equal_the_int64_convolution(integer_batches):
    for cases, xs, hs, out, ldo in integer_batches:
        for n, (K, L, p) in enumerate(cases):
            want = R.reverb_ref(xs[n].astype(np.int64), L, hs[n].astype(np.int64), p, ldo)
            assert np.abs(want).max() <= 2 ** 19
            assert np.array_equal(out[n].astype(np.int64), want) and np.all(out[n] == np.rint(out[n])), (K, L, p)
            assert np.all(out[n, L:] == 0)


def test_integer_longest_response():
    K, L = 16384, 2 * 16384 + 17
    rng = np.random.default_rng(2)
    cases = [(K, L, 5000), (K, L - 4000, K - 1)]
    xs, hs, out, ldo = run_batch(cases, int_x(rng), int_h(rng))
    for n, (K, L, p) in enumerate(cases):
        want = R.reverb_ref(xs[n].astype(np.int64), L, hs[n].astype(np.int64), p, ldo)
        assert np.array_equal(out[n].astype(np.int64), want), n
        assert np.any(want[:L] != 0)


# ---- 2. identities -------------------------------------------------------------------------------------------------------------
def rand_x(rng):
    def make(L):
        x = rng.uniform(-1.0, 1.0, L).astype(np.float32)
        return np.where(x == 0, np.float32(0.5), x)                           # the sum starts from +0: a -0 would come out as +0
    return make


def test_unit_responses_copy_bit_for_bit():
    t = tile()
    rng = np.random.default_rng(3)
    cases = [(1, t + 1, 0), (1, 33, 0), (40, 2 * t + 5, 17), (65, t - 1, 64), (1000, 700, 0), (2, 1, 1)]

    def delta(K):
        h = np.zeros(K, np.float32)
        h[delta.peaks.pop(0)] = 1.0
        return h
    delta.peaks = [p for _, _, p in cases]
    xs, hs, out, ldo = run_batch(cases, rand_x(rng), delta)
    for n, (K, L, p) in enumerate(cases):
        assert hs[n][p] == 1.0 and np.count_nonzero(hs[n]) == 1
        assert np.array_equal(out[n, :L].view(np.int32), xs[n].view(np.int32)), (K, L, p)
        assert np.all(out[n, L:].view(np.int32) == 0)


def test_rows_without_a_response_are_copied():
    t = tile()
    rng = np.random.default_rng(4)
    cases = [(33, t + 9, 3), (64, 100, 0), (5, 2 * t, 4), (7, 31, 2)]
    xs, hs, out, ldo = run_batch(cases, rand_x(rng), lambda K: rng.uniform(-1, 1, K).astype(np.float32), dry=(0, 3))
    for n in (0, 3):
        L = cases[n][1]
        assert np.array_equal(out[n, :L].view(np.int32), xs[n].view(np.int32)) and np.all(out[n, L:].view(np.int32) == 0)
    for n in (1, 2):
        assert not np.array_equal(out[n, :cases[n][1]], xs[n])


@pytest.mark.parametrize("wider", [True, False])
def test_a_null_rir_off_copies_the_batch_and_zeroes_the_rest(wider):
    """ldo > ldw and ldo < ldw: the columns from L to ldo are zero, the clip is cut at ldo."""
    o, t = ops(), tile()
    rng = np.random.default_rng(5)
    lens = [t + 40, 17, t - 1]
    ldw = t + 50
    ldo = ldw + 37 if wider else t + 3
    x = rng.uniform(-1, 1, (3, ldw)).astype(np.float32)
    out = torch.full((3, ldo), FILL, dtype=torch.float32, device="cuda")
    o.reverb(torch.from_numpy(x).cuda(), lens, None, None, None, None, out=out)
    got = out.cpu().numpy()
    for n, L in enumerate(lens):
        m = min(L, ldo)
        assert np.array_equal(got[n, :m].view(np.int32), x[n, :m].view(np.int32)) and np.all(got[n, m:].view(np.int32) == 0)
    # the same with responses: a different ldo changes nothing but where the row ends
    h = rng.uniform(-1, 1, 50).astype(np.float32)
    bank = torch.from_numpy(h).cuda()
    args = (torch.from_numpy(x).cuda(), lens, bank, np.zeros(3, np.int64), np.full(3, 50, np.int32), np.full(3, 7, np.int32))
    out.fill_(FILL)
    o.reverb(*args, out=out)
    base = o.reverb(*args).cpu().numpy()                                      # ldo = ldw
    got = out.cpu().numpy()
    for n, L in enumerate(lens):
        m = min(L, ldo)
        assert np.array_equal(got[n, :m].view(np.int32), base[n, :m].view(np.int32)) and np.all(got[n, m:].view(np.int32) == 0)
        assert np.all(base[n, L:] == 0) and np.any(base[n, :L] != x[n, :L])


# ---- 3. floats -----------------------------------------------------------------------------------------------------------------
def test_floats_stay_inside_the_fma_chain_bound():
    from deepspeech.pytorch_amd.augment import RirBank
    t = tile()
    rng = np.random.default_rng(6)
    taps = {K: RirBank.prepare(RirBank.synthetic_taps((K - 0.5) / 16000.0, rng, 0.0), "energy")[0] for K in KS + (4096,)}
    assert all(len(h) == K for K, h in taps.items())
    worst = {}
    extra = [[(4096, L, p) for L, p in zip((t + 1, 2 * t + 100, 777, t), (0, 1, 2048, 4095))]]
    for cases in seam_cases() + extra:
        xs, hs, out, ldo = run_batch(cases, lambda L: rng.uniform(-1, 1, L).astype(np.float32), lambda K: taps[K])
        for n, (K, L, p) in enumerate(cases):
            ref = R.reverb_ref(xs[n].astype(np.float64), L, hs[n].astype(np.float64), p, ldo)
            bound = 2.0 * K * 2.0 ** -24 * R.reverb_abs_ref(xs[n], L, hs[n], p, ldo)
            err = np.abs(out[n].astype(np.float64) - ref)
            worst[K] = max(worst.get(K, 0.0), float((err[:L] / bound[:L]).max()))
            assert np.all(bound[:L] > 0) and np.all(err <= bound), (K, L, p, float(err.max()))
    print("max |out - ref64| / bound per K:", {K: "%.3e" % v for K, v in sorted(worst.items())})
    assert worst[1000] > 0.0 and worst[4096] > 0.0                            # fp32 did round somewhere


# ---- 4. placement --------------------------------------------------------------------------------------------------------------
def test_a_clip_has_the_same_bits_wherever_it_sits():
    o, t = ops(), tile()
    rng = np.random.default_rng(7)
    L, K, p = 2 * t + 77, 1500, 40
    x = rng.uniform(-1, 1, L).astype(np.float32)
    h = (rng.standard_normal(K) * np.exp(-np.arange(K) / 300.0)).astype(np.float32)
    other = (rng.standard_normal(4000) * 0.1).astype(np.float32)
    bank1 = torch.from_numpy(h).cuda()
    alone = o.reverb(torch.from_numpy(x[None]).cuda(), [L], bank1, np.zeros(1, np.int64), np.array([K], np.int32),
                     np.array([p], np.int32)).cpu().numpy()[0]
    # row 5 of 8, among longer and shorter neighbours with other responses, another bank layout, other ldw / ldo
    lens = [3 * t, 5, L + 900, t, 31, L, 4 * t + 3, 100]
    ldw, ldo = max(lens) + 11, max(lens) + 300
    xb = rng.uniform(-1, 1, (8, ldw)).astype(np.float32)
    xb[5, :L] = x
    bank8 = torch.from_numpy(np.concatenate([other, h])).cuda()
    off = np.array([0, 0, -1, 0, 0, 4000, 0, -1], np.int64)
    ln = np.array([4000, 100, 0, 33, 4000, K, 2048, 0], np.int32)
    pk = np.array([0, 99, 0, 5, 3999, p, 7, 0], np.int32)
    out = torch.full((8, ldo), FILL, dtype=torch.float32, device="cuda")
    o.reverb(torch.from_numpy(xb).cuda(), lens, bank8, off, ln, pk, out=out)
    row = out.cpu().numpy()[5]
    assert np.array_equal(row[:L].view(np.int32), alone.view(np.int32)) and np.all(row[L:] == 0)
    assert np.any(alone != x)


# ---- 5. bounds -----------------------------------------------------------------------------------------------------------------
def test_a_response_reaching_past_the_bank_reads_zeros():
    o, t = ops(), tile()
    rng = np.random.default_rng(8)
    L, K, short = t + 50, 300, 120
    x = rng.integers(-8, 9, (2, L)).astype(np.float32)
    h = rng.integers(-4, 5, short).astype(np.float32)
    h[-1] = 2.0
    bank = torch.from_numpy(np.concatenate([np.full(7, 3.0, np.float32), h])).cuda()       # the bank ends `short` taps into the response
    out = torch.full((4, L + 4), FILL, dtype=torch.float32, device="cuda")
    o.reverb(torch.from_numpy(x).cuda(), [L, L - 9], bank, np.array([7, 7], np.int64), np.array([K, K], np.int32),
             np.array([0, 100], np.int32), out=out[1:3])
    got = out.cpu().numpy()
    assert np.all(got[0] == FILL) and np.all(got[3] == FILL)
    hp = np.concatenate([h, np.zeros(K - short, np.float32)]).astype(np.int64)
    for n, (Ln, p) in enumerate(((L, 0), (L - 9, 100))):
        assert np.array_equal(got[1 + n].astype(np.int64), R.reverb_ref(x[n].astype(np.int64), Ln, hp, p, L + 4))


# ---- 6. argument errors ----------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    from deepspeech.pytorch_amd import _lib
    o = ops()
    lib = _lib.load()
    N, ld = 2, 64
    x = torch.ones((N, ld), dtype=torch.float32, device="cuda")
    out = torch.full((N, ld), FILL, dtype=torch.float32, device="cuda")
    ns = torch.tensor([ld, 10], dtype=torch.int32, device="cuda")
    bank = torch.ones(8, dtype=torch.float32, device="cuda")
    off = torch.zeros(N, dtype=torch.int64, device="cuda")
    ln = torch.full((N,), 8, dtype=torch.int32, device="cuda")
    pk = torch.zeros(N, dtype=torch.int32, device="cuda")
    good = dict(wav=x, ldw=ld, ns=ns, N=N, bank=bank, blen=8, off=off, ln=ln, pk=pk, out=out, ldo=ld)

    def raw(**kw):
        a = dict(good, **kw)
        return lib.ds2_reverb(o.P(a["wav"]), a["ldw"], o.P(a["ns"]), a["N"], o.P(a["bank"]), a["blen"], o.P(a["off"]), o.P(a["ln"]),
                              o.P(a["pk"]), o.P(a["out"]), a["ldo"], o.S())

    bad = [dict(wav=None), dict(ns=None), dict(out=None), dict(out=x), dict(N=0), dict(N=-1), dict(N=65536), dict(ldw=0), dict(ldo=0),
           dict(ldo=-5), dict(bank=None), dict(ln=None), dict(pk=None)]
    for kw in bad:
        assert raw(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert torch.all(out == FILL) and torch.all(x == 1.0)
    assert raw() == 0 and raw(off=None, bank=None, ln=None, pk=None) == 0    # and the good calls are taken
    torch.cuda.synchronize()
    assert torch.all(out[0] == 1.0) and torch.all(out[1, :10] == 1.0) and torch.all(out[1, 10:] == 0.0)
    with pytest.raises(ValueError):
        o.reverb(x, ns, None, off, ln, pk)
    with pytest.raises(ValueError):
        o.reverb(x, ns, bank, off, ln[:1], pk)


# ---- 7. the front-end ----------------------------------------------------------------------------------------------------------
def clips(rng, lens):
    ld = max(lens) + 9
    wav = np.zeros((len(lens), ld), np.float32)
    for n, L in enumerate(lens):
        wav[n, :L] = rng.uniform(-0.5, 0.5, L).astype(np.float32)
    return torch.from_numpy(wav).cuda()


@pytest.fixture(scope="module")
def banks():
    from deepspeech.pytorch_amd.augment import NoiseBank, RirBank
    rng = np.random.default_rng(9)
    rirs = RirBank.synthetic([0.02, 0.11, 0.06], rng, drr_db=3.0)
    noise = NoiseBank.from_waveforms([rng.uniform(-0.3, 0.3, 30000).astype(np.float32), rng.uniform(-0.3, 0.3, 26000).astype(np.float32)])
    return rirs, noise


LENS = [20000, 4800, 12345, 16000, 1000]


def test_front_end_with_reverb_only(banks):
    from deepspeech.pytorch_amd.augment import WaveAugment
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    o = ops()
    rirs, _ = banks
    wav = clips(np.random.default_rng(10), LENS)
    fe = SpectrogramFrontEnd(wave_augment=WaveAugment(rir_bank=rirs, rir_prob=1.0), rng=np.random.default_rng(21))
    inputs, pct, frames = fe(wav, LENS)
    wd, offsets = fe.last_wave
    assert offsets is None and np.all(wd.rir_off >= 0) and len(set(wd.rir_off.tolist())) > 1
    plain = SpectrogramFrontEnd()
    wet = o.reverb(wav, LENS, rirs.samples, wd.rir_off, wd.rir_len, wd.rir_peak)
    want, pct0, frames0 = plain(wet, LENS)
    assert torch.equal(inputs, want) and torch.equal(pct, pct0) and torch.equal(frames, frames0)
    dry, pct1, frames1 = plain(wav, LENS)
    assert torch.equal(pct, pct1) and torch.equal(frames, frames1) and not torch.equal(inputs, dry)


def test_front_end_full_chain_and_collate(banks):
    from deepspeech.pytorch_amd.augment import WaveAugment
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    o = ops()
    rirs, noise = banks
    wav = clips(np.random.default_rng(11), LENS)
    make = lambda rb: WaveAugment(speed_volume_perturb=True, noise_bank=noise, noise_prob=0.7, rir_bank=rb, rir_prob=0.6)   # noqa: E731
    fe = SpectrogramFrontEnd(wave_augment=make(rirs), rng=np.random.default_rng(24))
    inputs, pct, frames = fe(wav, LENS)
    wd, offsets = fe.last_wave
    assert 0 < int((wd.rir_off >= 0).sum()) < len(LENS) and np.any(wd.noise_off >= 0)
    Lm, Smax = int(wd.nsamples.max()), int(wd.segments.max())
    w, ns_dev, offs = o.wsola(wav, LENS, wd.tempo, Lm, Smax)
    assert torch.equal(offs, offsets)
    w = o.reverb(w, ns_dev, rirs.samples, wd.rir_off, wd.rir_len, wd.rir_peak)
    w = o.wave_mix(w, ns_dev, wd.gain, wd.level, noise.samples, wd.noise_off, wd.noise_start)
    want, pct0, frames0 = SpectrogramFrontEnd()(w, wd.nsamples)
    assert torch.equal(inputs, want) and torch.equal(pct, pct0) and torch.equal(frames, frames0)
    # frame counts and percentages are those of the same tempo draws without the bank (reverberation keeps every length)
    from deepspeech.pytorch_amd.augment import WaveDraws
    bare = SpectrogramFrontEnd(wave_augment=make(None))
    dry = WaveDraws(wd.tempo, wd.gain, wd.gain_db, wd.level, wd.noise_off, wd.noise_start, wd.nsamples, wd.segments)
    dry_in, pct1, frames1 = bare._call_wave_augmented(wav, torch.tensor(LENS, dtype=torch.int32), False, dry)
    assert torch.equal(pct, pct1) and torch.equal(frames, frames1) and dry_in.shape == inputs.shape and not torch.equal(dry_in, inputs)
    # collate from the same seed: the same draws in the given order, sorted by length
    fe2 = SpectrogramFrontEnd(wave_augment=make(rirs), rng=np.random.default_rng(24))
    host = [wav[n, :L].cpu() for n, L in enumerate(LENS)]
    cin, cpct, order = fe2.collate(host)
    assert sorted(order) == list(range(len(LENS)))
    for r, n in enumerate(order):
        T = int(frames[n])
        assert torch.equal(cin[r, :, :, :T], inputs[n, :, :, :T])
    assert torch.equal(cpct, pct[order])


def test_front_end_with_probability_zero_equals_the_bankless_call(banks):
    """The binomial draw still happens with rir_prob = 0, so the bank-less front-end gets the draws of the restated order
    (WaveDraws of the call with the bank, its reverberation fields dropped), not its own RNG stream."""
    from deepspeech.pytorch_amd.augment import WaveAugment, WaveDraws, wsola_out_len
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    rirs, noise = banks
    wav = clips(np.random.default_rng(12), LENS)
    fe = SpectrogramFrontEnd(wave_augment=WaveAugment(speed_volume_perturb=True, noise_bank=noise, noise_prob=0.7, rir_bank=rirs,
                                                      rir_prob=0.0), rng=np.random.default_rng(23))
    inputs, pct, frames = fe(wav, LENS)
    wd, _ = fe.last_wave
    assert np.all(wd.rir_off == -1)
    want = R.draw_ref(LENS, np.random.default_rng(23), True, noise_bank=noise, noise_prob=0.7, rir_bank=rirs, rir_prob=0.0,
                      out_len=wsola_out_len)
    assert wd.nsamples.tolist() == want["nsamples"] and np.array_equal(wd.tempo, np.array(want["tempo"], np.float32))
    assert wd.noise_off.tolist() == [w[0] for w in want["noise"]] and wd.noise_start.tolist() == [w[2] for w in want["noise"]]
    bare = SpectrogramFrontEnd(wave_augment=WaveAugment(speed_volume_perturb=True, noise_bank=noise, noise_prob=0.7))
    dry = WaveDraws(wd.tempo, wd.gain, wd.gain_db, wd.level, wd.noise_off, wd.noise_start, wd.nsamples, wd.segments)
    ns = torch.tensor(LENS, dtype=torch.int32)
    inputs0, pct0, frames0 = bare._call_wave_augmented(wav, ns, False, dry)
    assert torch.equal(inputs, inputs0) and torch.equal(pct, pct0) and torch.equal(frames, frames0)


def test_streaming_refuses_a_front_end_that_reverberates(banks):
    from deepspeech.pytorch_amd.augment import WaveAugment
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    fe = SpectrogramFrontEnd(normalize="running", wave_augment=WaveAugment(rir_bank=banks[0]))
    with pytest.raises(ValueError, match="wave_augment"):
        fe.stream(2, "cuda")
