"""Host-side checks of per-clip sample rates (no GPU): the bank's classes and refusals, the streaming plan per class against the
definition restated in numpy (tests/resample_reference.py), the speed-to-class mapping and the order of the draws."""
import ctypes

import numpy as np
import pytest

import resample_reference as RR
from deepspeech.pytorch_amd import _lib
from deepspeech.pytorch_amd.augment import WaveAugment, speed_rate
from deepspeech.pytorch_amd.resample import MAX_CLASSES, Resampler, ResamplerBank
from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd

RATES = (8000, 16000, 48000, 44100, 11025)


def test_a_bank_holds_the_designs_of_its_resamplers_back_to_back():
    bank = ResamplerBank(RATES)
    table = bank.classes.reshape(len(RATES), 10)
    off = 0
    for c, r in enumerate(RATES):
        rs = Resampler(r)
        U, D, W = (1, 1, 0) if r == 16000 else RR.params(r)
        assert table[c, :3].tolist() == [U, D, W] == [rs.up, rs.down, rs.half_width]
        assert int(table[c, 8:10].copy().view(np.int64)[0]) == off and off % 2 == 0
        assert np.array_equal(bank.taps[off:off + U * 2 * W].reshape(U, 2 * W), rs.taps)          # design_taps' bits
        assert np.array_equal(bank.resampler(r).taps, rs.taps) and bank.class_of[r] == c
        if W:
            assert bank.tile(r) == _lib.query("ds2_resample_tile", U, D, W) == table[c, 6]
            assert table[c, 7] * 4 <= 44 * 1024                                                   # the LDS budget of a workgroup
        off += U * 2 * W
    assert bank.taps.size == off and bank.half_width == 72
    assert [bank.out_len(4410, r) for r in RATES] == [RR.out_len(4410, *RR.params(r)[:2]) for r in RATES]
    assert bank.out_len(4410, 16000) == 4410


def test_the_class_table_helper_refuses_what_the_entries_refuse():
    tab, total = np.zeros(17 * 10, np.int32), ctypes.c_long(0)
    H = lambda a: ctypes.c_void_p(a.ctypes.data)                                                  # noqa: E731
    ok = np.array([(2, 1, 24), (1, 1, 0)], np.int32)
    _lib.call("ds2_resample_classes", H(ok), 2, H(tab), ctypes.byref(total))
    assert total.value == 96
    for udw, C in ((ok, 0), (np.tile(ok, (9, 1))[:17], 17), (np.array([(16384, 1, 24)], np.int32), 1), (np.array([(1, 1, -1)], np.int32), 1),
                   (np.array([(2, 1, 0)], np.int32), 1), (np.array([(0, 1, 24)], np.int32), 1)):
        with pytest.raises(_lib.Ds2HipError, match="1002"):
            _lib.call("ds2_resample_classes", H(np.ascontiguousarray(udw)), C, H(tab), ctypes.byref(total))
    with pytest.raises(_lib.Ds2HipError, match="1002"):
        _lib.call("ds2_resample_classes", ctypes.c_void_p(0), 2, H(tab), ctypes.byref(total))


def test_bank_refusals_name_the_rate():
    with pytest.raises(ValueError, match="48510 Hz"):
        ResamplerBank([16000, 48510])                                                             # 44100 x 1.1: a table of 912 KiB
    with pytest.raises(ValueError, match="at most 16 rates"):
        ResamplerBank([8000 + 1000 * k for k in range(MAX_CLASSES + 1)])
    assert len(ResamplerBank([8000 + 1000 * k for k in range(MAX_CLASSES)]).rates) == 16
    with pytest.raises(ValueError, match="distinct"):
        ResamplerBank([8000, 8000])
    for bad in ([], [0], [-8000], [8000.5]):
        with pytest.raises(ValueError, match="positive integer"):
            ResamplerBank(bad)
    bank = ResamplerBank([8000, 16000])
    for call in (lambda: bank.out_len(10, 22050), lambda: bank.plan_resample(22050, 0, 10), lambda: bank.resampler(8000.5),
                 lambda: bank.stream(2, "cpu").reset([0], [44100])):
        with pytest.raises(ValueError, match="not a rate of this bank"):
            call()
    st = bank.stream(2, "cpu")
    with pytest.raises(ValueError, match="2 rates for 1 slots"):
        st.reset([0], [8000, 16000])
    st.reset([1], 8000)
    assert st.rates == [None, 8000]
    st.reset()                                                                                    # keeps the rates
    assert st.rates == [None, 8000]


@pytest.mark.parametrize("rate", RATES)
def test_plan_resample_per_class_is_the_definitions_plan(rate):
    bank = ResamplerBank(RATES)
    U, D, W = RR.params(rate)
    rng = np.random.RandomState(rate)
    G = 0
    for k in range(60):
        n = int(rng.choice([0, 1, W - 1, W, W + 1, 2 * W, 97, 1000]))
        final = k == 59
        got = tuple(bank.plan_resample(rate, G, n, final))
        assert got == tuple(Resampler(rate).plan_resample(G, n, final))
        if rate == 16000:
            assert got == (G, n, 0, 0, G)                                                         # the copy class: nothing is carried
        else:
            assert got == RR.plan(G, n, final, U, D, W)
        G += n


def test_speed_times_rate_is_exact_and_maps_to_the_class_of_the_product():
    assert [speed_rate(16000, s) for s in (0.9, 1.0, 1.1)] == [14400, 16000, 17600]
    assert [speed_rate(48000, s) for s in (0.9, 1.0, 1.1)] == [43200, 48000, 52800]
    assert [speed_rate(8000, s) for s in (0.9, 1.0, 1.1)] == [7200, 8000, 8800]
    assert 48000 * 1.1 != 52800                                                                   # what the float product gives
    with pytest.raises(ValueError, match="11025 Hz at speed 0.9"):
        speed_rate(11025, 0.9)                                                                    # 9922.5 Hz
    wa = WaveAugment(speed_choices=(0.9, 1.0, 1.1))
    fe = SpectrogramFrontEnd(wave_augment=wa, input_rate=(48000, 16000, 8000))
    assert set(fe.bank.rates) == {43200, 48000, 52800, 14400, 16000, 17600, 7200, 8000, 8800}
    for r in (48000, 16000, 8000):
        for s in (0.9, 1.0, 1.1):
            rs = fe.bank.resampler(speed_rate(r, s))
            want = RR.params(speed_rate(r, s)) if speed_rate(r, s) != 16000 else (1, 1, 0)        # on 48 kHz: 10/27, 1/3, 10/33
            assert (rs.up, rs.down, rs.half_width) == want
    assert fe.bank.resampler(16000).identity                                                      # speed 1.0 on 16 kHz: the copy class
    assert (fe.bank.resampler(43200).up, fe.bank.resampler(43200).down) == (10, 27)
    one = SpectrogramFrontEnd(wave_augment=wa)                                                    # input_rate None: 16 kHz x speeds
    assert one.bank.rates == (14400, 16000, 17600) and one.rates is None and one.resampler is None
    with pytest.raises(ValueError, match="44100 Hz at speed 1.1"):                                # 48510 Hz: U = 1600, 912 KiB
        SpectrogramFrontEnd(wave_augment=WaveAugment(speed_choices=(1.0, 1.1)), input_rate=(16000, 44100))
    with pytest.raises(ValueError, match="44100 Hz at speed 0.9"):
        SpectrogramFrontEnd(wave_augment=wa, input_rate=44100)
    with pytest.raises(ValueError, match="11025 Hz at speed 0.9"):
        SpectrogramFrontEnd(wave_augment=wa, input_rate=(11025,))
    plain = SpectrogramFrontEnd(input_rate=44100)                                                 # what was there stays what it was
    assert plain.bank is None and plain.rates is None and plain.resampler.in_rate == 44100
    assert SpectrogramFrontEnd(input_rate=(16000, 8000)).rates == (16000, 8000)
    for bad in ((), (8000, 8000), (8000.5,), (0,)):
        with pytest.raises(ValueError, match="distinct positive integer"):
            SpectrogramFrontEnd(input_rate=bad)
    with pytest.raises(ValueError, match="positive factors"):
        WaveAugment(speed_choices=(0.9, 0.0))


class Recorder:
    """a numpy Generator that writes down which draws were asked of it"""

    def __init__(self, seed):
        self.rng, self.calls = np.random.default_rng(seed), []

    def __getattr__(self, name):
        def draw(*a, **kw):
            self.calls.append(name)
            return getattr(self.rng, name)(*a, **kw)
        return draw


def test_the_speed_is_the_first_draw_of_a_clip_and_nothing_else_moves():
    lens, rates = [20000, 48000, 9000], [16000, 48000, 8000]
    wa = WaveAugment(speed_volume_perturb=True, speed_choices=(0.9, 1.0, 1.1))
    rec = Recorder(3)
    wd = wa.draw(lens, rec, rates=rates)
    assert rec.calls == ["choice", "uniform", "uniform"] * 3
    # replayed by hand: the choice, then the reference's tempo and gain draws on the resampled length
    rng = np.random.default_rng(3)
    from deepspeech.pytorch_amd.augment import wsola_out_len
    for n in range(3):
        s = (0.9, 1.0, 1.1)[int(rng.choice(3))]
        tempo = float("%.3f" % rng.uniform(low=0.85, high=1.15))
        gain = float("%.3f" % rng.uniform(low=-6, high=8))
        eff = speed_rate(rates[n], s)
        n16 = -((-lens[n] * 16000) // eff)
        assert (wd.speed[n], wd.rates[n], wd.resampled[n]) == (s, eff, n16) == (s, eff, Resampler(eff).out_len(lens[n]))
        assert wd.tempo[n] == np.float32(tempo) and wd.gain_db[n] == gain and wd.nsamples[n] == wsola_out_len(n16, tempo)
    took = wd.take([2, 0])
    assert took.speed.tolist() == wd.speed[[2, 0]].tolist() and took.rates.tolist() == wd.rates[[2, 0]].tolist()
    # without speed_choices every configuration draws what it drew
    a = WaveAugment(speed_volume_perturb=True).draw(lens, np.random.default_rng(4))
    rec = Recorder(4)
    b = WaveAugment(speed_volume_perturb=True, speed_choices=None).draw(lens, rec)
    assert rec.calls == ["uniform", "uniform"] * 3 and b.speed is None and b.rates is None and b.resampled is None
    assert a.tempo.tolist() == b.tempo.tolist() and a.gain_db.tolist() == b.gain_db.tolist() and a.nsamples.tolist() == b.nsamples.tolist()
    assert not WaveAugment().active and WaveAugment(speed_choices=(1.0,)).active
    with pytest.raises(ValueError, match="belongs to speed_choices"):
        WaveAugment(speed_volume_perturb=True).draw(lens, np.random.default_rng(4), rates=rates)
    with pytest.raises(ValueError, match="rates has 2 entries"):
        wa.draw(lens, np.random.default_rng(4), rates=[16000, 8000])
