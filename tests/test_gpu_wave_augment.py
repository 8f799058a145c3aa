"""GPU checks of the waveform augmentation kernels (csrc/ds2_waveaug.hip: k_wsola, k_wave_energy, k_wave_mix) and of
SpectrogramFrontEnd(wave_augment=...) against the outputs of the real reference in tests/golden/waveaug and the fp64 restatement
tests/wave_augment_reference.py.  Every batch runs once, in a module-scoped fixture.

Mix: the yardstick is the fp32 noise of the reference itself, as in tests/test_gpu_spec_augment.py: a device output may differ
from the reference output by 4 x the fixture's recorded max |fp64 restatement - reference| plus 4 * eps_fp32 * max |x|.
WSOLA: (1) with the offsets the device reports, its output equals the restatement forced to those offsets to 4 * eps_fp32 * max |x|
(the cross-fade is one subtraction and one fused multiply-add per sample, 2.5 eps in all); (2) every reported offset's fp64 dot
product is within the recorded margin (4 x the fp32 error numpy's own evaluation shows on these inputs,
tests/golden/waveaug/README.md) of its segment's fp64 maximum; (3) where that maximum is unique by more than the margin
(asserted on the CPU in tests/test_wave_augment_host.py) the offsets equal the fp64 arg-max, no exemptions."""
import ctypes as C
import glob
import json
import os

import numpy as np
import pytest
import torch

import wave_augment_reference as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "waveaug")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)
HOP = 160
FILL = 7.0                                                  # what the output buffers hold before a kernel runs


def noise():
    with open(os.path.join(GOLDEN, "reference_noise.json")) as f:
        return json.load(f)


# ---- gain + noise mix against the golden fixtures --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    """all fixtures side by side in ONE padded batch with one noise bank (the recordings back to back); the energy kernel runs
    twice (determinism), the mix once into a buffer pre-filled with FILL.  name -> (fixture, out row, energy partials (8, 2))."""
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd.augment import NoiseBank
    zs = {n: dict(np.load(os.path.join(GOLDEN, n + ".npz"))) for n in FIXTURES}
    with_noise = [n for n in FIXTURES if len(zs[n]["noise"])]
    bank = NoiseBank.from_waveforms([zs[n]["noise"] for n in with_noise])
    N, ld = len(FIXTURES), max(len(z["data"]) for z in zs.values()) + 1
    x = np.full((N, ld), 0.25, np.float32)                  # the input's padding is not zero either: nothing may read it
    gain, level = np.ones(N, np.float32), np.zeros(N, np.float32)
    off, start = np.full(N, -1, np.int64), np.zeros(N, np.int32)
    lens = []
    for k, n in enumerate(FIXTURES):
        z = zs[n]
        L = len(z["data"])
        lens.append(L)
        if "gain_db" in z:
            x[k, :L], gain[k] = z["raw"], R.gain_factor(float(z["gain_db"]))
        else:
            x[k, :L] = z["data"]
        level[k], start[k] = float(z["level"]), int(z["start"])
        if n in with_noise:
            off[k] = bank.offsets[with_noise.index(n)]
    xd = torch.from_numpy(x).cuda()
    args = (xd, lens, gain, level, bank.samples, off, start)
    p1 = ops.wave_energy(*args)
    p2 = ops.wave_energy(*args)
    out = torch.full((N, ld), FILL, dtype=torch.float32, device="cuda")
    ops.wave_mix(*args, partial=p1, out=out)
    assert torch.equal(p1, p2), "the energy partials differ between two launches"
    assert np.array_equal(xd.cpu().numpy(), x)               # out of place
    out, p1 = out.cpu().numpy(), p1.cpu().numpy()
    return {n: (zs[n], out[k], p1[k]) for k, n in enumerate(FIXTURES)}


def test_mix_batch_covers_the_shapes(mixed):
    lens = {len(z["data"]) for z, _, _ in mixed.values()}
    assert {1, 255, 256, 257, 2047, 2048, 2049} <= lens      # 256 = a workgroup's share, 2048 = one sweep of the energy kernel
    starts = {(int(z["start"]), len(z["noise"]) - len(z["data"])) for z, _, _ in mixed.values() if len(z["noise"])}
    assert any(s == 0 for s, _ in starts) and any(s == room and room > 0 for s, room in starts)
    assert next(iter(mixed.values()))[2].shape == (8, 2)


@pytest.mark.parametrize("name", FIXTURES)
def test_mix_matches_the_reference_output(mixed, name):
    z, out, partial = mixed[name]
    L = len(z["data"])
    allowed = 4 * noise()[name] + 4 * EPS32 * float(np.abs(z["data"]).max())
    err = float(np.abs(out[:L].astype(np.float64) - z["out"]).max())
    print("%s: max |device - golden| = %.3e, allowed %.3e" % (name, err, allowed))
    assert np.all(out[L:] == 0)                              # the buffer held FILL there
    assert err <= allowed
    if name.startswith("hand_"):                             # no noise for the clip / a crop without energy: the clip itself
        assert np.array_equal(out[:L], z["data"])
    elif "gain_db" in z:
        assert float(np.abs(z["raw"]).max()) > 1.0 / float(R.gain_factor(float(z["gain_db"])))    # the gain did clamp
    else:
        assert np.any(out[:L] != z["data"])


@pytest.mark.parametrize("name", FIXTURES)
def test_energy_partials_sum_to_the_fp64_energies(mixed, name):
    """fp64 sums of exactly representable squares in another order: n * eps_fp64 relative."""
    z, _, partial = mixed[name]
    L, s = len(z["data"]), int(z["start"])
    has = len(z["noise"]) > 0 and float(z["level"]) > 0
    ed, en = R.energies(z["data"], z["noise"][s:s + L] if has else np.zeros(L))
    got = partial.sum(0)
    assert abs(got[0] - ed) <= L * EPS64 * ed and abs(got[1] - en) <= L * EPS64 * en
    used = min(8, -(-L // 256))                              # block b sums the samples i with (i / 256) % 8 == b
    assert np.all(partial[used:] == 0) and np.all(partial[:used, 0] > 0)


# ---- WSOLA -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stretched():
    """wsola_cases(): the first five as one batch (N = 5, different lengths and tempi side by side), the last alone (N = 1).
    name -> (x, tempo, out row, reported sample count, offsets row)."""
    from deepspeech.pytorch_amd import ops
    cases = R.wsola_cases()
    res = {}
    for group in (cases[:5], cases[5:]):
        N, ld = len(group), max(len(x) for _, x, _, _ in group) + 3
        buf = np.full((N, ld), 0.25, np.float32)
        for k, (_, x, _, _) in enumerate(group):
            buf[k, :len(x)] = x
        lens = [len(x) for _, x, _, _ in group]
        tempo = np.array([t for _, _, t, _ in group], np.float32)
        ldo = max(R.out_len(L, t) for L, t in zip(lens, tempo)) + 5
        Smax = max(R.segments(L, t) for L, t in zip(lens, tempo)) + 2
        out = torch.full((N, ldo), FILL, dtype=torch.float32, device="cuda")
        _, ns_out, offsets = ops.wsola(torch.from_numpy(buf).cuda(), lens, tempo, ldo, Smax, out=out)
        out, ns_out, offsets = out.cpu().numpy(), ns_out.cpu().numpy(), offsets.cpu().numpy()
        for k, (name, x, t, _) in enumerate(group):
            res[name] = (x, float(tempo[k]), out[k], int(ns_out[k]), offsets[k])
    return res


NAMES = [c[0] for c in R.wsola_cases()]
UNIQUE = [c[0] for c in R.wsola_cases() if c[3]]


@pytest.mark.parametrize("name", NAMES)
def test_wsola_output_equals_the_restatement_at_the_reported_offsets(stretched, name):
    x, tempo, out, n_out, offsets = stretched[name]
    S = R.segments(len(x), tempo)
    assert n_out == R.out_len(len(x), tempo)
    assert np.all(offsets[S:] == -1) and np.all(offsets[:S] >= 0) and np.all(offsets[:S] < R.SEARCH) and (S == 0 or offsets[0] == 0)
    want, _ = R.wsola(x, tempo, offsets=offsets[:S])
    err = float(np.abs(out[:n_out].astype(np.float64) - want).max())
    allowed = 4 * EPS32 * float(np.abs(x).max())
    print("%s: S %d, %d -> %d samples, offsets %s, max |device - f64| %.3e, allowed %.3e" % (name, S, len(x), n_out, offsets[:S].tolist(), err, allowed))
    assert err <= allowed
    assert np.all(out[n_out:] == 0)                          # the buffer held FILL there
    if S == 0:
        assert np.array_equal(out[:n_out], x)                # copied unchanged


@pytest.mark.parametrize("name", NAMES)
def test_wsola_offsets_are_maxima_to_the_fp32_margin(stretched, name):
    x, tempo, _, _, offsets = stretched[name]
    margin = noise()["wsola_dot_margin"]
    prev = 0
    for k in range(1, R.segments(len(x), tempo)):
        d = R.dots(x, prev, k, tempo)
        assert d[offsets[k]] >= d.max() - margin, (name, k, int(offsets[k]), int(np.argmax(d)), d.max() - d[offsets[k]])
        if d.max() == d.min():
            assert offsets[k] == 0                           # every candidate ties: the lowest offset
        prev = R.start(k, tempo) + int(offsets[k])


@pytest.mark.parametrize("name", UNIQUE)
def test_wsola_offsets_equal_the_fp64_argmax_where_it_is_unique(stretched, name):
    x, tempo, out, n_out, offsets = stretched[name]
    want, chosen = R.wsola(x, tempo)
    assert offsets[:len(chosen)].tolist() == chosen.tolist()
    assert float(np.abs(out[:n_out] - want).max()) <= 4 * EPS32 * float(np.abs(x).max())


def test_wsola_zero_stretch_ties_go_to_the_lowest_offset(stretched):
    x, tempo, _, _, offsets = stretched["zero_stretch"]
    _, chosen = R.wsola(x, tempo)
    assert offsets[:len(chosen)].tolist() == chosen.tolist()  # the segments outside the stretch are unique by far more than the margin
    tails = [k for k in range(1, len(chosen)) if not x[R.start(k - 1, tempo) + int(chosen[k - 1]) + R.ADV:][:R.OVL].any()]
    assert len(tails) >= 2 and all(offsets[k] == 0 for k in tails)


# ---- the front-end ---------------------------------------------------------------------------------------------------------
LENS = [6000, 5003, 1500]


def waveforms():
    buf = torch.zeros((len(LENS), max(LENS)))
    for k, n in enumerate(LENS):
        buf[k, :n] = torch.from_numpy(R.chirp_noise(n, 20 + k, amp=0.3))
    return buf.cuda()


def noise_bank():
    from deepspeech.pytorch_amd.augment import NoiseBank
    rs = np.random.RandomState(12)
    return NoiseBank.from_waveforms([(0.1 * rs.standard_normal(n)).astype(np.float32) for n in (9000, 7000)])


def raw_spectrogram(fe, wav, ns_dev, N, Lm, aug=None):
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd._lib import call, query
    out = torch.full((N, 1, 161, 1 + Lm // HOP), 5.0, dtype=torch.float32, device=wav.device)
    ws = torch.empty(query("ds2_spect_ws_bytes", N, Lm), dtype=torch.uint8, device=wav.device)
    head = (ops.P(wav), wav.stride(0), ops.P(ns_dev), N, Lm, ops.P(fe._basis_on(wav.device)), 1 if fe.reflect else 0,
            1 if fe.normalize else 0, ops.P(out), ops.P(ws))
    if aug is None:
        call("ds2_spectrogram", *head, ops.S())
    else:
        warp, W, fm, tm = aug
        coef = torch.empty((N, 3), dtype=torch.float32, device=wav.device)
        call("ds2_spectrogram_aug", *head, ops.P(warp), W, ops.P(fm), fm.shape[1], ops.P(tm), tm.shape[1], ops.P(coef), ops.S())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("augment", [False, True])
def test_front_end_equals_the_kernels_chained_by_hand(augment):
    """seeded rng: the same draws by hand, ds2_wsola -> ds2_wave_energy + ds2_wave_mix -> ds2_spectrogram(_aug), bit for bit;
    frame counts and percentages are those of the lengths after the tempo change."""
    from deepspeech.pytorch_amd import configs, ops
    from deepspeech.pytorch_amd.augment import SpecAugment, WaveAugment
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    bank = noise_bank()
    wa = WaveAugment(speed_volume_perturb=True, noise_bank=bank, noise_prob=0.7)
    sa = SpecAugment(time_masking_para=10)
    fe = SpectrogramFrontEnd(configs.SpectConfig(), spec_augment=sa, wave_augment=wa, rng=np.random.default_rng(3))
    wav = waveforms()
    got, pct, frames = fe(wav, LENS, augment=augment)
    rng = np.random.default_rng(3)
    wd = wa.draw(LENS, rng)
    assert wd.nsamples.tolist() == [R.out_len(L, t) for L, t in zip(LENS, wd.tempo)] and wd.nsamples.tolist() != LENS
    assert (wd.noise_off >= 0).any()
    Lm = int(wd.nsamples.max())
    want_frames = 1 + wd.nsamples // HOP
    assert frames.tolist() == want_frames.tolist()
    assert torch.equal(pct, (torch.from_numpy(want_frames).double() / float(1 + Lm // HOP)).float())
    assert got.shape == (3, 1, 161, 1 + Lm // HOP)
    y, ns_dev, offsets = ops.wsola(wav, LENS, wd.tempo, Lm, int(wd.segments.max()))
    assert ns_dev.cpu().tolist() == wd.nsamples.tolist()
    assert torch.equal(offsets, fe.last_wave[1])
    z = ops.wave_mix(y, ns_dev, wd.gain, wd.level, bank.samples, wd.noise_off, wd.noise_start)
    aug = None
    if augment:
        warp, fm, tm = sa.draw(want_frames, 161, rng)
        aug = (torch.from_numpy(warp).cuda(), sa.W, torch.from_numpy(fm).cuda(), torch.from_numpy(tm).cuda())
    want = raw_spectrogram(fe, z, ns_dev, 3, Lm, aug)
    assert torch.equal(got, want)
    assert torch.isfinite(got).all()
    plain, _, plain_frames = SpectrogramFrontEnd(configs.SpectConfig())(wav, LENS)
    assert plain.shape != got.shape or not torch.equal(plain, got)


def test_front_end_without_wave_augment_is_unchanged():
    from deepspeech.pytorch_amd import configs
    from deepspeech.pytorch_amd.augment import WaveAugment
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    wav = waveforms()
    base = SpectrogramFrontEnd(configs.SpectConfig(), rng=np.random.default_rng(1))
    for wa in (None, WaveAugment()):                         # None, and one with every step off
        fe = SpectrogramFrontEnd(configs.SpectConfig(), rng=np.random.default_rng(1), wave_augment=wa)
        base.rng = np.random.default_rng(1)
        for augment in (False, True):
            a, pa, fa = base(wav, LENS, augment=augment)
            b, pb, fb = fe(wav, LENS, augment=augment)
            assert torch.equal(a, b) and torch.equal(pa, pb) and torch.equal(fa, fb)
        assert fe.last_wave is None
    ns_dev = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    assert torch.equal(base(wav, LENS)[0], raw_spectrogram(base, wav, ns_dev, 3, max(LENS)))


def test_collate_sorts_by_the_length_after_the_tempo_change():
    from deepspeech.pytorch_amd import configs
    from deepspeech.pytorch_amd.augment import WaveAugment
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    lens = [5000, 5200, 5100]                                # close enough for the tempo draws to reorder them
    wavs = [torch.from_numpy(R.chirp_noise(n, 30 + k, amp=0.3)) for k, n in enumerate(lens)]
    wa = WaveAugment(speed_volume_perturb=True)
    for seed in range(50):
        wd = wa.draw(lens, np.random.default_rng(seed))
        order = sorted(range(3), key=lambda i: -int(wd.nsamples[i]))
        if order != [1, 2, 0]:
            break
    else:
        raise AssertionError("no seed reorders the clips")
    fe = SpectrogramFrontEnd(configs.SpectConfig(), wave_augment=wa, rng=np.random.default_rng(seed))
    inputs, pct, got_order = fe.collate(wavs)
    assert got_order == order
    frames = 1 + np.sort(wd.nsamples)[::-1] // HOP
    assert inputs.shape == (3, 1, 161, int(frames[0])) and pct[0] == 1.0
    assert torch.equal(pct, (torch.from_numpy(frames.copy()).double() / float(frames[0])).float())
    # the same clips, already in that order, through __call__ with the permuted draws' seed: row r of collate = clip order[r]
    buf = torch.zeros((3, max(lens)))
    for r, i in enumerate(order):
        buf[r, :lens[i]] = wavs[i]
    again = fe._call_wave_augmented(buf.cuda(), torch.tensor([lens[i] for i in order], dtype=torch.int32), False, wd.take(order))[0]
    assert torch.equal(inputs, again)


def test_argument_errors():
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd._lib import load
    lib, st, null = load(), ops.S(), C.c_void_p(0)
    x = torch.zeros((2, 2000), device="cuda")
    out = torch.empty((2, 2400), device="cuda")
    ns = torch.tensor([2000, 1800], dtype=torch.int32, device="cuda")
    tp = torch.ones(2, device="cuda")
    nso = torch.empty(2, dtype=torch.int32, device="cuda")
    offs = torch.empty((2, 4), dtype=torch.int32, device="cuda")
    ok = (ops.P(x), 2000, ops.P(ns), ops.P(tp), 2, ops.P(out), 2400, ops.P(nso), ops.P(offs), 4, st)
    assert lib.ds2_wsola(*ok) == 0
    assert lib.ds2_wsola(ops.P(x), 2000, ops.P(ns), null, 2, ops.P(out), 2400, ops.P(nso), null, 0, st) == 0      # no tempo: a copy
    assert torch.equal(out[:, :2000], x) and nso.cpu().tolist() == [2000, 1800]
    for i, bad in ((0, null), (2, null), (5, null), (7, null), (5, ops.P(x)), (4, 0), (6, 0), (9, -1), (8, null)):
        args = list(ok)
        args[i] = bad
        assert lib.ds2_wsola(*args) != 0, i
    lv = torch.full((2,), 0.3, device="cuda")
    bank = torch.ones(5000, device="cuda")
    off = torch.zeros(2, dtype=torch.int64, device="cuda")
    start = torch.zeros(2, dtype=torch.int32, device="cuda")
    ws = torch.empty((2, 8, 2), dtype=torch.float64, device="cuda")
    mo = torch.empty_like(x)
    e_ok = (ops.P(x), 2000, ops.P(ns), 2, null, ops.P(lv), ops.P(bank), 5000, ops.P(off), ops.P(start), ops.P(ws), st)
    assert lib.ds2_wave_energy(*e_ok) == 0
    for i, bad in ((0, null), (2, null), (3, 0), (6, null), (7, 0), (8, null), (9, null), (10, null)):
        args = list(e_ok)
        args[i] = bad
        assert lib.ds2_wave_energy(*args) != 0, i
    m_ok = e_ok[:11] + (ops.P(mo), 2000, st)
    assert lib.ds2_wave_mix(*m_ok) == 0
    for i, bad in ((0, null), (2, null), (3, 0), (6, null), (10, null), (11, null), (11, ops.P(x)), (12, 0)):
        args = list(m_ok)
        args[i] = bad
        assert lib.ds2_wave_mix(*args) != 0, i
    assert lib.ds2_wave_mix(ops.P(x), 2000, ops.P(ns), 2, null, null, null, 0, null, null, null, ops.P(mo), 2000, st) == 0   # a plain copy
    assert torch.equal(mo[1, :1800], x[1, :1800]) and not mo[1, 1800:].any()
    with pytest.raises(ValueError):
        ops.wave_mix(x, [2000], None)
    with pytest.raises(ValueError):
        ops.wave_mix(x, [2000, 1800], None, lv)                           # levels without a bank
    with pytest.raises(ValueError):
        ops.wsola(x.cpu(), [2000, 1800], tp, 2400, 4)
    torch.cuda.synchronize()
