"""GPU checks of SpecAugment on the device (csrc/ds2_spect.hip: k_spect_warp_coef, k_spect_write<true>, k_spec_augment) against
the outputs of the real reference in tests/golden/specaug and the fp64 restatement tests/spec_augment_reference.py.

The yardstick is the fp32 noise of the reference itself: tests/golden/specaug/reference_noise.json holds, per fixture,
max |fp64 restatement - reference output|.  A device output may differ from the reference output by 4 x that figure plus
4 * eps_fp32 * max |x| (the device adds one more fp32 rounding of the same kind).  That ds2_spectrogram itself is unchanged is
what tests/test_gpu_spect.py checks, unmodified."""
import ctypes as C
import glob
import json
import os

import numpy as np
import pytest
import torch

import spec_augment_reference as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "specaug")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
EPS32 = float(np.finfo(np.float32).eps)
HOP = 160


def noise():
    with open(os.path.join(GOLDEN, "reference_noise.json")) as f:
        return json.load(f)


def bound(figure, x):
    return 4 * figure + 4 * EPS32 * float(np.abs(x).max())


def warp_draw_of(z):
    return np.concatenate([[float(z["i"]), float(z["d"])], z["E"], [0.0]]).astype(np.float32)


@pytest.fixture(scope="module")
def batches():
    """the fixtures grouped by bin count into padded batches (clips of different T side by side), each run ONCE through the
    standalone entry with the recorded coefficients and through the coefficient kernel: name -> (fixture, output, coefficients)."""
    from deepspeech.pytorch_amd import ops
    zs = {n: dict(np.load(os.path.join(GOLDEN, n + ".npz"))) for n in FIXTURES}
    res = {}
    for F in sorted({z["x"].shape[0] for z in zs.values()}):
        names = [n for n in FIXTURES if zs[n]["x"].shape[0] == F]
        Tmax = max(zs[n]["x"].shape[1] for n in names)
        x = np.full((len(names), 1, F, Tmax), 7.0, np.float32)           # the padding is NOT zero: the kernel has to write it
        fm = np.zeros((len(names), 4, 2), np.int32)
        tm = np.zeros((len(names), 4, 2), np.int32)
        for k, n in enumerate(names):
            z = zs[n]
            x[k, 0, :, :z["x"].shape[1]] = z["x"]
            fm[k, :len(z["fmask"])], tm[k, :len(z["tmask"])] = z["fmask"], z["tmask"]
        frames = [zs[n]["x"].shape[1] for n in names]
        xd = torch.from_numpy(x).cuda()
        coef_ref = np.stack([zs[n]["coef_ref"] for n in names]).astype(np.float32)
        out = ops.spec_augment(xd, frames, torch.from_numpy(coef_ref), torch.from_numpy(fm), torch.from_numpy(tm)).cpu().numpy()
        coef = ops.spec_augment_coef(xd, frames, torch.from_numpy(np.stack([warp_draw_of(zs[n]) for n in names]))).cpu().numpy()
        assert np.array_equal(xd.cpu().numpy(), x)                        # out of place
        for k, n in enumerate(names):
            res[n] = (zs[n], out[k, 0], coef[k])
    return res


@pytest.mark.parametrize("name", FIXTURES)
def test_standalone_matches_the_reference_output(batches, name):
    z, out, _ = batches[name]
    F, T = z["x"].shape
    err = float(np.abs(out[:, :T].astype(np.float64) - z["out"]).max())
    print("%s: max |device - golden| = %.3e, allowed %.3e" % (name, err, bound(noise()[name], z["x"])))
    assert np.all(out[:, T:] == 0)                                        # frames >= frames[n]
    assert np.all(out[:, :T][R.in_mask(F, T, z["fmask"], z["tmask"])] == 0)
    assert np.any(out[:, :T] != 0)
    assert err <= bound(noise()[name], z["x"])


@pytest.mark.parametrize("name", FIXTURES)
def test_coefficient_kernel_is_as_close_to_exact_as_the_reference(batches, name):
    z, _, dev = batches[name]
    F, T = z["x"].shape
    exact = R.warp_coef(F, T, z["pt"], int(z["i"]), int(z["d"]), z["E"])
    allowed = np.maximum(np.abs(z["coef_ref"] - exact), 1e-6 * np.abs(exact))
    print("%s: |dev - f64| %s allowed %s" % (name, np.abs(dev - exact), allowed))
    assert np.all(np.abs(dev.astype(np.float64) - exact) <= allowed)


def test_coefficient_kernel_switches(batches):
    """no warp: negative i, i >= T, T <= 2W, a singular block (non-finite solution)."""
    from deepspeech.pytorch_amd import ops
    x = torch.from_numpy(np.random.RandomState(3).standard_normal((5, 1, 9, 30)).astype(np.float32)).cuda()
    E = np.random.RandomState(4).standard_normal(9) / 1e10
    d = np.zeros((5, 12), np.float32)
    d[:, 1], d[:, 2:11] = 2, E
    d[:, 0] = [-1, 12, 25, 6, 12]
    d[4, 2:11] = 0
    coef = ops.spec_augment_coef(x, [30, 30, 20, 10, 30], torch.from_numpy(d)).cpu().numpy()
    assert not coef[0].any() and coef[1].any() and not coef[2].any() and not coef[3].any() and not coef[4].any()
    assert np.all(np.isfinite(coef))
    assert np.allclose(coef[1], R.warp_coef(9, 30, float(x[1, 0, 4, 12]), 12, 2, E), rtol=1e-6, atol=0)


LENS = [64 * HOP, 63 * HOP + 7, 11 * HOP + 5]            # 65, 64 and 12 frames


def waveforms():
    rs = np.random.RandomState(11)
    buf = torch.zeros((len(LENS), max(LENS)))
    for k, n in enumerate(LENS):
        buf[k, :n] = torch.from_numpy((rs.standard_normal(n) * rs.uniform(0.05, 0.5)).astype(np.float32))
    return buf.cuda()


def raw_spectrogram(fe, wav, lens, aug=None):
    """ds2_spectrogram, or ds2_spectrogram_aug with aug = (warp_draw or None, W, fmask or None, MF, tmask or None, MT)."""
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd._lib import call, query
    N, Lm = len(lens), max(lens)
    out = torch.full((N, 1, 161, 1 + Lm // HOP), 5.0, dtype=torch.float32, device=wav.device)
    ws = torch.empty(query("ds2_spect_ws_bytes", N, Lm), dtype=torch.uint8, device=wav.device)
    ns = torch.tensor(lens, dtype=torch.int32, device=wav.device)
    head = (ops.P(wav), wav.stride(0), ops.P(ns), N, Lm, ops.P(fe._basis_on(wav.device)), 1 if fe.reflect else 0,
            1 if fe.normalize else 0, ops.P(out), ops.P(ws))
    if aug is None:
        call("ds2_spectrogram", *head, ops.S())
        return out, None
    warp, W, fm, MF, tm, MT = aug
    coef = torch.full((N, 3), 9.0, dtype=torch.float32, device=wav.device)
    call("ds2_spectrogram_aug", *head, ops.P(warp), W, ops.P(fm), MF, ops.P(tm), MT, ops.P(coef), ops.S())
    torch.cuda.synchronize()
    return out, coef


@pytest.mark.parametrize("W", [5, 6])
def test_fused_equals_standalone_on_the_plain_spectrogram(W):
    """T = 65, 64, 12: with W = 6 the third clip has T <= 2W and gets masks only; with the reference's W = 5 it is warped.  The
    generator seed is the first whose draw makes clip 1's query frames run past ITS last frame (chosen with the fp64 restatement
    from the plain spectrogram), so a clamp against Tmax - 2 = 63 instead of its own T - 2 = 62 would show."""
    from deepspeech.pytorch_amd import configs, ops
    from deepspeech.pytorch_amd.augment import SpecAugment
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    sa = SpecAugment(frequency_mask_num=2, time_mask_num=2, time_masking_para=20, W=W)
    fe = SpectrogramFrontEnd(configs.SpectConfig(), spec_augment=sa)
    wav = waveforms()
    frames = [1 + n // HOP for n in LENS]
    plain, _, _ = fe(wav, LENS)
    p = plain.cpu().numpy()
    for seed in range(1000):
        warp, fm, tm = sa.draw(frames, 161, np.random.default_rng(seed))
        cf = [R.warp_coef(161, T, p[k, 0, 80, max(int(warp[k, 0]), 0)], int(warp[k, 0]), int(warp[k, 1]), warp[k, 2:11], W=W)
              for k, T in enumerate(frames)]
        flow = [np.abs(c) @ np.array([160.0, T - 1, 1.0]) for c, T in zip(cf, frames)]
        q1 = np.arange(64)[None, :] - (cf[1][0] * np.arange(161)[:, None] + cf[1][1] * np.arange(64)[None, :] + cf[1][2])
        unmasked_last = tm[1, :, 0].max() + 20 < 60
        if all(f <= 2 * T for f, T in zip(flow, frames)) and q1[:, -1].max() > 64.5 and unmasked_last and cf[0].any():
            break
    else:
        raise AssertionError("no draw found")
    fe.rng = np.random.default_rng(seed)
    fused, pct, fr = fe(wav, LENS, augment=True)
    coef = fe.last_coef
    assert fr.tolist() == frames
    alone = ops.spec_augment(plain, frames, coef, torch.from_numpy(fm), torch.from_numpy(tm))
    fused, alone, coef = fused.cpu().numpy(), alone.cpu().numpy(), coef.cpu().numpy()
    assert (coef[2].any()) == (W == 5)                                    # T = 12 <= 2 * 6
    for k, T in enumerate(frames):
        assert np.allclose(coef[k], cf[k], rtol=1e-4, atol=1e-6), (k, coef[k], cf[k])     # pt is an fp32 device value
        allowed = bound(noise()["e2e_f161_t%d" % T], p[k, 0, :, :T])
        err = float(np.abs(fused[k, 0].astype(np.float64) - alone[k, 0]).max())
        want = R.spec_augment(p[k, 0, :, :T], coef[k], fm[k], tm[k])
        err64 = float(np.abs(fused[k, 0, :, :T] - want).max())
        print("W %d clip %d (T %d): |fused - standalone| %.3e, |fused - f64| %.3e, allowed %.3e" % (W, k, T, err, err64, allowed))
        assert err <= allowed and err64 <= allowed
        assert np.all(fused[k, 0, :, T:] == 0)
        assert np.all(fused[k, 0, :, :T][R.in_mask(161, T, fm[k], tm[k])] == 0)
    # clip 1 clamped against Tmax - 2 would read its frame 64 (zero padding of the plain batch) instead of holding frame 63
    wrong = R.spec_augment(p[1, 0, :, :65], coef[1], fm[1], tm[1])[:, :64]
    assert np.abs(wrong - fused[1, 0, :, :64]).max() > 100 * bound(noise()["e2e_f161_t64"], p[1, 0])


def test_fused_without_warp_and_masks_is_the_plain_spectrogram():
    from deepspeech.pytorch_amd import configs
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    fe = SpectrogramFrontEnd(configs.SpectConfig())
    wav = waveforms()
    plain, _ = raw_spectrogram(fe, wav, LENS)
    zero = torch.zeros((3, 4, 2), dtype=torch.int32, device=wav.device)
    zero[:, :, 0] = 3                                                     # a start without a width masks nothing
    for aug in ((None, 5, zero, 4, zero, 4), (None, 5, None, 0, None, 0)):
        out, coef = raw_spectrogram(fe, wav, LENS, aug)
        assert torch.equal(out, plain)
        assert not coef.any()
    off = torch.zeros((3, 12), dtype=torch.float32, device=wav.device)
    off[:, 0], off[:, 1], off[:, 2:11] = -1, 3, 1e-10
    out, coef = raw_spectrogram(fe, wav, LENS, (off, 5, None, 0, None, 0))
    assert torch.equal(out, plain) and not coef.any()


def test_front_end_without_augment_is_unchanged():
    from deepspeech.pytorch_amd import configs
    from deepspeech.pytorch_amd.augment import SpecAugment
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    wav = waveforms()
    fe = SpectrogramFrontEnd(configs.SpectConfig(), spec_augment=SpecAugment(time_mask_num=2), rng=np.random.default_rng(0))
    raw, _ = raw_spectrogram(fe, wav, LENS)
    a, pct_a, fr_a = fe(wav, LENS)
    b, pct_b, fr_b = fe(wav, LENS, augment=False)
    assert torch.equal(a, raw) and torch.equal(b, raw) and torch.equal(pct_a, pct_b) and torch.equal(fr_a, fr_b)
    assert fe.last_coef is None
    c, pct_c, fr_c = fe(wav, LENS, augment=True)
    assert torch.equal(pct_c, pct_a) and torch.equal(fr_c, fr_a) and not torch.equal(c, raw) and torch.isfinite(c).all()
    wavs = [wav[k, :n].cpu() for k, n in enumerate(LENS)]
    plain = fe.collate(wavs)
    assert torch.equal(plain[0], raw) and plain[2] == [0, 1, 2]
    aug = fe.collate(wavs, augment=True)
    assert aug[0].shape == raw.shape and torch.equal(aug[1], plain[1]) and not torch.equal(aug[0], raw)


def test_argument_errors():
    from deepspeech.pytorch_amd import configs, ops
    from deepspeech.pytorch_amd._lib import Ds2HipError, load
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    x = torch.zeros((2, 1, 9, 20), device="cuda")
    coef = torch.zeros((2, 3))
    m5 = torch.zeros((2, 5, 2), dtype=torch.int32)
    m1 = torch.zeros((2, 1, 2), dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.spec_augment(x, [20, 20], coef, m5, None)
    with pytest.raises(ValueError):
        ops.spec_augment(x, [20, 20], coef, None, m5)
    with pytest.raises(ValueError):
        ops.spec_augment(x, [20], coef, None, None)
    with pytest.raises(ValueError):
        ops.spec_augment(x, [20, 20], coef[:1], None, None)
    with pytest.raises(ValueError):
        ops.spec_augment(x, [20, 20], coef, m1[:1], None)
    with pytest.raises(ValueError):
        ops.spec_augment(x.cpu(), [20, 20], coef, None, None)
    with pytest.raises(ValueError):
        ops.spec_augment_coef(x, [20, 20], torch.zeros((2, 11)))
    assert torch.equal(ops.spec_augment(x + 1, [20, 3], coef, None, m1)[1, 0, :, 3:], x[1, 0, :, 3:])
    # the raw ABI
    lib, st = load(), ops.S()
    fr, cf, out = torch.tensor([20, 20], dtype=torch.int32).cuda(), coef.cuda(), torch.empty_like(x)
    m5d, null = m5.cuda(), C.c_void_p(0)
    ok = lambda *a: lib.ds2_spec_augment(*a)                              # noqa: E731
    assert ok(ops.P(x), ops.P(out), 2, 9, 20, ops.P(fr), ops.P(cf), null, 0, null, 0, st) == 0
    for args in ((null, ops.P(out), 2, 9, 20, ops.P(fr), ops.P(cf), null, 0, null, 0, st),
                 (ops.P(x), null, 2, 9, 20, ops.P(fr), ops.P(cf), null, 0, null, 0, st),
                 (ops.P(x), ops.P(x), 2, 9, 20, ops.P(fr), ops.P(cf), null, 0, null, 0, st),          # in place
                 (ops.P(x), ops.P(out), 2, 9, 20, null, ops.P(cf), null, 0, null, 0, st),
                 (ops.P(x), ops.P(out), 2, 9, 20, ops.P(fr), null, null, 0, null, 0, st),
                 (ops.P(x), ops.P(out), 2, 9, 20, ops.P(fr), ops.P(cf), null, 1, null, 0, st),         # masks announced, none given
                 (ops.P(x), ops.P(out), 2, 9, 20, ops.P(fr), ops.P(cf), null, 0, null, 1, st),
                 (ops.P(x), ops.P(out), 2, 9, 20, ops.P(fr), ops.P(cf), ops.P(m5d), 5, null, 0, st),
                 (ops.P(x), ops.P(out), 2, 9, 20, ops.P(fr), ops.P(cf), null, 0, ops.P(m5d), 5, st),
                 (ops.P(x), ops.P(out), 0, 9, 20, ops.P(fr), ops.P(cf), null, 0, null, 0, st),
                 (ops.P(x), ops.P(out), 2, 0, 20, ops.P(fr), ops.P(cf), null, 0, null, 0, st)):
        assert ok(*args) != 0
    assert lib.ds2_spec_augment_coef(ops.P(x), 2, 9, 20, ops.P(fr), null, 5, null, st) != 0
    assert lib.ds2_spec_augment_coef(null, 2, 9, 20, ops.P(fr), null, 5, ops.P(cf), st) != 0
    fe = SpectrogramFrontEnd(configs.SpectConfig())
    wav = waveforms()
    m5w = torch.zeros((3, 5, 2), dtype=torch.int32, device="cuda")
    for aug in ((None, 5, m5w, 5, None, 0), (None, 5, None, 0, m5w, 5), (None, 5, None, 1, None, 0), (None, -1, None, 0, None, 0)):
        with pytest.raises(Ds2HipError):
            raw_spectrogram(fe, wav, LENS, aug)
    torch.cuda.synchronize()
