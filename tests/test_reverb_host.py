"""CPU-side checks of the reverberation (run with -m "not gpu"): augment.RirBank's rules against their restatement in
tests/reverb_reference.py, WaveAugment.draw with and without a rir_bank against the restated draw order, the new WaveDraws fields,
and that the kernel is declared and built."""
import itertools
import math
import os
import re

import numpy as np
import pytest

import reverb_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def aug():
    from deepspeech.pytorch_amd import augment
    return augment


# ---- the bank ------------------------------------------------------------------------------------------------------------------
def test_peak_is_the_first_argmax():
    A = aug()
    h = [0.0, 0.25, -1.0, 0.5, 1.0, -1.0, 0.1]                       # |h| = 1 at 2, 4 and 5
    bank = A.RirBank.from_waveforms([h, [3.0], [0.0, 0.0, -2.0, 2.0]], device="cpu", normalize=None)
    assert bank.peaks.tolist() == [2, 0, 2] and bank.peaks.dtype == np.int32
    assert len(bank) == 3 and [bank.length(r) for r in range(3)] == [7, 1, 4]
    assert bank.offsets.tolist() == [0, 7, 8, 12] and bank.offsets.dtype == np.int64
    assert np.array_equal(bank.samples.numpy(), np.array(h + [3.0] + [0.0, 0.0, -2.0, 2.0], np.float32))
    assert R.prepare_ref(h, None)[1] == 2


@pytest.mark.parametrize("normalize", ["energy", "peak", None])
@pytest.mark.parametrize("max_taps", [5, 40, 41, 16384])
def test_cut_and_normalisation_match_the_restatement(normalize, max_taps):
    A = aug()
    rng = np.random.default_rng(7)
    irs = []
    for n, p in ((40, 0), (41, 4), (200, 3)):
        h = rng.standard_normal(n) * np.exp(-np.arange(n) / 30.0)
        h[p] = 3.0 * (-1) ** p                                       # the peak, kept by every cut tried here
        irs.append(h)
    bank = A.RirBank.from_waveforms(irs, device="cpu", normalize=normalize, max_taps=max_taps)
    s = bank.samples.numpy()
    assert s.dtype == np.float32
    for r, h in enumerate(irs):
        want, p = R.prepare_ref(h, normalize, max_taps)
        got = s[bank.offsets[r]:bank.offsets[r + 1]]
        assert bank.length(r) == min(len(h), max_taps) == len(want) and bank.peaks[r] == p
        assert np.array_equal(got, want)                             # fp64 on the host, rounded to fp32 once: the same bits
        g = got.astype(np.float64)
        if normalize == "energy":
            assert abs(float((g * g).sum()) - 1.0) <= len(g) * 2.0 ** -23
        elif normalize == "peak":
            assert abs(g[p]) == 1.0
        else:
            assert np.array_equal(got, h[:max_taps].astype(np.float32))


def test_refusals():
    A = aug()
    make = lambda irs, **kw: A.RirBank.from_waveforms(irs, device="cpu", **kw)      # noqa: E731
    for bad in ([], [[]], [[0.0, 0.0]], [[1.0], np.zeros(5)]):
        with pytest.raises(ValueError):
            make(bad)
    h = np.zeros(10)
    h[6] = 1.0
    assert make([h], max_taps=7).length(0) == 7                      # the peak is the last tap kept
    with pytest.raises(ValueError, match="max_taps"):
        make([h], max_taps=6)                                        # the peak AT max_taps
    with pytest.raises(ValueError, match="max_taps"):
        make([h], max_taps=3)
    with pytest.raises(ValueError):
        make([h], normalize="rms")
    with pytest.raises(ValueError):
        R.prepare_ref(h, None, 6)


@pytest.mark.parametrize("rt60,drr_db", [(0.05, 0.0), (0.128, 6.0), (0.3001, 3.0)])
def test_synthetic_direct_path_and_tail_energy(rt60, drr_db):
    A = aug()
    h = A.RirBank.synthetic_taps(rt60, np.random.default_rng(3), drr_db)
    assert len(h) == math.ceil(rt60 * 16000) and h[0] == 1.0         # unit direct path before normalisation
    assert abs(float((h[1:] ** 2).sum()) - 10.0 ** (-drr_db / 10.0)) <= 1e-12
    assert np.array_equal(h, R.synthetic_ref(rt60, np.random.default_rng(3), drr_db))
    env = np.exp(-3.0 * math.log(10.0) * np.arange(1, len(h)) / (rt60 * 16000))
    g = h[1:] / env                                                  # a * standard normal draws under a 60 dB decay over rt60
    assert np.all(np.abs(g) <= 6.0 * g.std()) and abs(g.mean()) <= 0.2 * g.std()
    for normalize in ("energy", "peak", None):
        bank = A.RirBank.synthetic([rt60, rt60], np.random.default_rng(3), drr_db, device="cpu", normalize=normalize)
        rng = np.random.default_rng(3)
        for r in range(2):                                           # one response per rt60, drawn one after the other
            want, p = R.prepare_ref(R.synthetic_ref(rt60, rng, drr_db), normalize)
            assert np.array_equal(bank.samples.numpy()[bank.offsets[r]:bank.offsets[r + 1]], want) and bank.peaks[r] == p
    assert A.RirBank.synthetic([1.5], np.random.default_rng(0), 6.0, device="cpu", max_taps=4096).length(0) == 4096


# ---- the draws -----------------------------------------------------------------------------------------------------------------
NS = [40000, 1000, 23456, 16000, 31999, 8000]
FIELDS = ("tempo", "gain", "gain_db", "level", "noise_off", "noise_start", "nsamples", "segments", "speed", "rates", "resampled")


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.dtype == b.dtype and np.array_equal(a, b))


@pytest.mark.parametrize("svp,noisy,speeds", list(itertools.product([False, True], [False, True], [None, (0.9, 1.0, 1.1)])))
def test_without_a_rir_bank_every_configuration_draws_what_it_drew(svp, noisy, speeds):
    A = aug()
    nb = R.FakeBank([50000, 30000, 64000]) if noisy else None
    old = A.WaveAugment(speed_volume_perturb=svp, noise_bank=nb, noise_prob=0.6, speed_choices=speeds)
    new = A.WaveAugment(speed_volume_perturb=svp, noise_bank=nb, noise_prob=0.6, speed_choices=speeds, rir_bank=None, rir_prob=0.9)
    assert old.active == new.active == (svp or noisy or bool(speeds))
    r1, r2 = np.random.default_rng(11), np.random.default_rng(11)
    a, b = old.draw(NS, r1), new.draw(NS, r2)
    for f in FIELDS:
        assert same(getattr(a, f), getattr(b, f)), f
    assert b.rir_off is None and b.rir_len is None and b.rir_peak is None and b.rir_arrays() == [None, None, None]
    assert r1.random() == r2.random()                                # the streams stand at the same place
    # and the draws are those of the restated order without its reverberation step
    if not speeds:
        want = R.draw_ref(NS, np.random.default_rng(11), svp, noise_bank=nb, noise_prob=0.6, out_len=A.wsola_out_len)
        check_against(b, want, nb, None)


def check_against(wd, want, nb, rb):
    N = len(want["nsamples"])
    assert wd.nsamples.tolist() == want["nsamples"]
    if want["tempo"][0] is None:
        assert wd.tempo is None and wd.gain is None and wd.gain_db is None
    else:
        assert np.array_equal(wd.tempo, np.array(want["tempo"], np.float32)) and wd.gain_db.tolist() == want["gain_db"]
        assert np.array_equal(wd.gain, np.power(10.0, np.array(want["gain_db"]) / 20.0).astype(np.float32))
    if nb is None:
        assert wd.level is None and wd.noise_off is None and wd.noise_start is None
    else:
        assert wd.noise_off.tolist() == [w[0] for w in want["noise"]]
        assert np.array_equal(wd.level, np.array([w[1] for w in want["noise"]], np.float32))
        assert wd.noise_start.tolist() == [w[2] for w in want["noise"]]
    if rb is None:
        assert wd.rir_off is None
    else:
        assert wd.rir_off.dtype == np.int64 and wd.rir_len.dtype == np.int32 and wd.rir_peak.dtype == np.int32
        for n in range(N):
            r = want["rir"][n]
            exp = (-1, 0, 0) if r < 0 else (int(rb.offsets[r]), rb.length(r), int(rb.peaks[r]))
            assert (int(wd.rir_off[n]), int(wd.rir_len[n]), int(wd.rir_peak[n])) == exp


@pytest.mark.parametrize("svp,noisy,prob", [(True, True, 0.5), (False, True, 0.5), (True, False, 0.3), (False, False, 1.0), (True, True, 0.0)])
def test_with_a_rir_bank_the_draws_follow_the_restated_order(svp, noisy, prob):
    A = aug()
    nb = R.FakeBank([50000, 30000, 64000]) if noisy else None
    rb = R.FakeBank([100, 2000, 7, 16384], peaks=[0, 13, 6, 200])
    wa = A.WaveAugment(speed_volume_perturb=svp, noise_bank=nb, noise_prob=0.6, rir_bank=rb, rir_prob=prob)
    assert wa.active
    ns = NS * 3
    wd = wa.draw(ns, np.random.default_rng(5))
    want = R.draw_ref(ns, np.random.default_rng(5), svp, noise_bank=nb, noise_prob=0.6, rir_bank=rb, rir_prob=prob, out_len=A.wsola_out_len)
    check_against(wd, want, nb, rb)
    if 0.0 < prob < 1.0:
        assert 0 < sum(r >= 0 for r in want["rir"]) < len(ns)
    elif prob == 1.0:
        assert all(r >= 0 for r in want["rir"]) and len(set(want["rir"])) > 1
    else:
        assert all(r < 0 for r in want["rir"])
    # RandomState has the same calls
    wd2 = wa.draw(ns, np.random.RandomState(5))
    check_against(wd2, R.draw_ref(ns, np.random.RandomState(5), svp, noise_bank=nb, noise_prob=0.6, rir_bank=rb, rir_prob=prob,
                                  out_len=A.wsola_out_len), nb, rb)


def test_from_config_takes_the_bank_and_the_probability():
    A = aug()
    rb = R.FakeBank([10])

    class Cfg:
        speed_volume_perturb, noise_dir = True, ""

    wa = A.WaveAugment.from_config(Cfg(), rir_bank=rb)
    assert wa.rir_bank is rb and wa.rir_prob == 0.5 and wa.speed_volume_perturb
    Cfg.rir_prob = 0.25
    assert A.WaveAugment.from_config(Cfg(), rir_bank=rb).rir_prob == 0.25
    assert A.WaveAugment.from_config(Cfg()).rir_bank is None


def test_arrays_rir_arrays_and_take():
    A = aug()
    rb = R.FakeBank([100, 2000, 7], peaks=[0, 13, 6])
    wa = A.WaveAugment(speed_volume_perturb=True, noise_bank=R.FakeBank([50000, 64000]), noise_prob=0.7, rir_bank=rb, rir_prob=0.7)
    wd = wa.draw(NS, np.random.default_rng(2))
    arrays = wd.arrays()
    assert len(arrays) == 5 and all(a is b for a, b in zip(arrays, (wd.noise_off, wd.tempo, wd.gain, wd.level, wd.noise_start)))
    rir = wd.rir_arrays()
    assert len(rir) == 3 and all(a is b for a, b in zip(rir, (wd.rir_off, wd.rir_len, wd.rir_peak)))
    assert len(set(wd.rir_off.tolist())) > 1
    order = [4, 0, 5, 2, 1, 3]
    t = wd.take(order)
    for f in FIELDS + ("rir_off", "rir_len", "rir_peak"):
        a, b = getattr(wd, f), getattr(t, f)
        assert same(None if a is None else a[order], b), f
    # the constructor takes the new fields by keyword, at the end, defaulting to None
    old = A.WaveDraws(wd.tempo, wd.gain, wd.gain_db, wd.level, wd.noise_off, wd.noise_start, wd.nsamples, wd.segments)
    assert old.rir_arrays() == [None, None, None] and old.take(order).rir_off is None
    kw = A.WaveDraws(wd.tempo, wd.gain, wd.gain_db, wd.level, wd.noise_off, wd.noise_start, wd.nsamples, wd.segments,
                     rir_off=wd.rir_off, rir_len=wd.rir_len, rir_peak=wd.rir_peak)
    assert kw.rir_arrays()[0] is wd.rir_off


# ---- the build -----------------------------------------------------------------------------------------------------------------
def test_the_kernel_is_declared_and_built():
    from deepspeech.pytorch_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "ds2hip.h")).read()
    assert re.search(r"^int ds2_reverb_tile\(void\);", header, re.M)
    assert re.search(r"^int ds2_reverb\(const float\* wav, long ldw, const int\* nsamples, int N,", header, re.M)
    assert "ds2_reverb.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ds2_reverb.hip"))
    assert "ds2_reverb" in _lib.SIGNATURES and "ds2_reverb_tile" in _lib.SIGNATURES
    tile = _lib.query("ds2_reverb_tile")
    assert tile >= 1024 and tile % 1024 == 0                         # whole 32 x 32 output matrices
