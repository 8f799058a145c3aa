"""CPU-side checks of the waveform augmentation (run with -m "not gpu"): the fp64 restatement tests/wave_augment_reference.py
against the outputs of the real reference in tests/golden/waveaug, WaveAugment.draw against a recorded numpy RandomState sequence
in the reference's order, the host-only length queries of the library against their Python mirror, and the properties of the
WSOLA rules that need no device (identity at tempo 1, the length bound, the uniqueness the GPU tests rely on)."""
import glob
import json
import os

import numpy as np
import pytest

import wave_augment_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "waveaug")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
EPS32 = float(np.finfo(np.float32).eps)


def noise():
    with open(os.path.join(GOLDEN, "reference_noise.json")) as f:
        return json.load(f)


def test_the_fixture_set_is_complete():
    assert {"len1", "len255", "len256", "len257", "len2047", "len2048", "len2049", "gain_clamps", "hand_no_noise",
            "hand_silent_crop"} <= set(FIXTURES)
    for n in FIXTURES:
        assert len(np.load(os.path.join(GOLDEN, n + ".npz"))["data"]) <= 4000


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_the_reference_output(name):
    """The recorded figure IS max |restatement - reference|; what is asserted is that it is fp32 rounding noise of the reference's
    own evaluation (a few ulp of the largest output), that the recorded fp32 and fp64 scale factors agree to fp32 precision, and
    that the gain restatement reproduces the fixture's gained data bit for bit."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    data, start, level = z["data"], int(z["start"]), float(z["level"])
    crop = z["noise"][start:start + len(data)] if len(z["noise"]) else None
    got = R.mix(data, crop, level)
    err = float(np.abs(got - z["out"]).max())
    assert err == pytest.approx(noise()[name], abs=1e-12)
    assert err <= 4 * EPS32 * float(np.abs(z["out"]).max())
    assert abs(float(z["scale32"]) - float(z["scale64"])) <= 4 * EPS32 * abs(float(z["scale64"]))
    if crop is not None:
        assert float(z["scale64"]) == R.scale(data, crop, level)
    if name.startswith("hand_"):
        assert np.array_equal(got, data)                                  # no noise / a silent crop: the clip itself
    if "gain_db" in z.files:
        assert np.array_equal(R.gain(z["raw"], float(z["gain_db"])), data)
        assert float(np.abs(data).max()) == 1.0


class FakeBank:
    """the two things draw() asks of a NoiseBank, without a device."""

    def __init__(self, lengths):
        self.offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)

    def __len__(self):
        return len(self.offsets) - 1

    def length(self, r):
        return int(self.offsets[r + 1] - self.offsets[r])


def test_draw_follows_the_reference_order():
    """Per clip: uniform (tempo), uniform (gain), binomial, and only for a clip that gets noise choice, uniform (level), rand --
    the calls of load_randomly_augmented_audio (data_loader.py:399-401), parse_audio (:157), inject_noise (:114-115) and
    inject_noise_sample (:121), replayed here on a RandomState with the same seed."""
    from deepspeech.pytorch_amd.augment import WaveAugment, wsola_out_len, wsola_segments
    bank = FakeBank([40000, 9000, 64000])
    wa = WaveAugment(speed_volume_perturb=True, noise_bank=bank, noise_prob=0.6, noise_levels=(0.1, 0.4))
    ns = [16000, 48000, 8000, 30000, 1000, 52000, 64000, 20000]
    g = np.random.RandomState(7)
    wd = wa.draw(ns, g)
    rs = np.random.RandomState(7)
    hit = 0
    for n, L in enumerate(ns):
        tempo = np.float32(float("%.3f" % rs.uniform(low=0.85, high=1.15)))                 # '{:.3f}'.format(tempo), :383
        gain = float("%.3f" % rs.uniform(low=-6, high=8))
        assert wd.tempo[n] == tempo and wd.gain_db[n] == gain
        assert wd.gain[n] == np.float32(10.0 ** (gain / 20.0))
        assert wd.nsamples[n] == wsola_out_len(L, tempo) == R.out_len(L, tempo)
        assert wd.segments[n] == wsola_segments(L, tempo) == R.segments(L, tempo)
        if rs.binomial(1, 0.6):
            r = rs.choice(3)
            level = rs.uniform(0.1, 0.4)
            u = rs.rand()
            room = bank.length(r) - int(wd.nsamples[n])
            if room < 0:                                                                    # longer than its recording: no noise
                assert wd.noise_off[n] == -1 and wd.level[n] == 0
                continue
            hit += 1
            assert wd.noise_off[n] == bank.offsets[r] and wd.level[n] == np.float32(level)
            assert 0 <= wd.noise_start[n] <= room and abs(int(wd.noise_start[n]) - u * room) <= 1
        else:
            assert wd.noise_off[n] == -1 and wd.level[n] == 0
    assert 0 < hit < len(ns)
    assert g.rand() == rs.rand()                                          # both consumed the same number of values
    # switches: nothing is drawn for a step that is off
    off = WaveAugment().draw(ns, np.random.RandomState(0))
    assert off.tempo is None and off.gain is None and off.level is None and off.nsamples.tolist() == ns
    assert not WaveAugment().active and wa.active
    only_noise = WaveAugment(noise_bank=bank, noise_prob=1.0).draw([100, 100000], np.random.RandomState(1))
    assert only_noise.tempo is None and only_noise.noise_off[0] >= 0 and only_noise.noise_off[1] == -1      # longer than every recording


def test_from_config_reads_the_five_fields():
    from types import SimpleNamespace
    from deepspeech.pytorch_amd.augment import WaveAugment
    cfg = SimpleNamespace(speed_volume_perturb=True, spec_augment=False, noise_dir="/data/noise", noise_prob=0.7, noise_min=0.2,
                          noise_max=0.3)
    with pytest.raises(ValueError):
        WaveAugment.from_config(cfg)                                      # noise_dir set, no bank given
    bank = FakeBank([100])
    wa = WaveAugment.from_config(cfg, bank)
    assert wa.speed_volume_perturb and wa.noise_bank is bank and wa.noise_prob == 0.7 and wa.noise_levels == (0.2, 0.3)
    assert wa.tempo_range == (0.85, 1.15) and wa.gain_range == (-6, 8)   # load_randomly_augmented_audio's defaults
    cfg.noise_dir, cfg.speed_volume_perturb = "", False
    wa = WaveAugment.from_config(cfg, bank)
    assert wa.noise_bank is None and not wa.active


def test_library_length_queries_equal_the_python_mirror():
    from deepspeech.pytorch_amd import _lib, build
    from deepspeech.pytorch_amd.augment import wsola_out_len, wsola_segments
    build.build(verbose=False)
    lib = _lib.load()
    rs = np.random.RandomState(3)
    lengths = list(range(1500, 1560)) + [1, 0, 1311, 1312, 1545, 1546, 240000, 2 ** 24 + 1] + rs.randint(1546, 300000, 300).tolist()
    tempi = [0.85, 1.0, 1.15, 0.1, 10.0, 0.0999, 10.5, 1.5, float("nan"), 0.851, 1.149] + rs.uniform(0.85, 1.15, 20).round(3).tolist()
    checked = 0
    for L in lengths:
        for t in tempi:
            want = (R.segments(L, t), R.out_len(L, t))
            assert (wsola_segments(L, t), wsola_out_len(L, t)) == want, (L, t)
            assert (lib.ds2_wsola_segments(L, t), lib.ds2_wsola_out_len(L, t)) == want, (L, t)
            checked += 1
    assert checked > 10000
    assert lib.ds2_wsola_segments(1545, 1.0) == 0 and lib.ds2_wsola_segments(1546, 1.0) == 2
    assert lib.ds2_wave_ws_bytes(3) == 3 * 8 * 2 * 8


def test_output_length_bound():
    """out_len lies within one segment of nsamples / tempo (and equals nsamples at tempo 1)."""
    rs = np.random.RandomState(5)
    for L in [1546, 1547, 2000, 16000, 240000] + rs.randint(1546, 300000, 200).tolist():
        assert R.out_len(L, 1.0) == L
        for t in (0.85, 0.9, 1.1, 1.15, 0.5, 2.0):
            assert abs(R.out_len(L, t) - L / float(np.float32(t))) <= R.SEG, (L, t)
            S = R.segments(L, t)
            assert R.start(S - 1, t) + R.OVL <= L < R.start(S, t) + R.OVL


@pytest.mark.parametrize("period", [32, 16, 8])
def test_identity_at_tempo_one_for_a_period_that_divides_the_hop(period):
    """The period divides 1120 and 192: every candidate window holds whole periods, offset 0 reproduces the tail exactly and
    attains the maximum, later multiples of the period tie with it and lose to the lowest offset; the cross-fade of equal samples
    is exact."""
    rs = np.random.RandomState(period)
    x = np.tile(rs.uniform(-0.5, 0.5, period), 6000 // period + 1)[:6000].astype(np.float32)
    out, chosen = R.wsola(x, 1.0)
    assert len(chosen) == 6 and not chosen.any()
    assert np.array_equal(out, x.astype(np.float64))


def test_forced_offsets_and_copy_rules():
    x = R.chirp_noise(4000, 9)
    out, chosen = R.wsola(x, 1.15)
    forced, again = R.wsola(x, 1.15, offsets=chosen)
    assert np.array_equal(out, forced) and np.array_equal(chosen, again)
    other, _ = R.wsola(x, 1.15, offsets=[0, 5, 7])
    assert len(other) == len(out) and not np.array_equal(other, out)
    for L, t in ((1545, 1.15), (4000, 0.05), (4000, 11.0), (4000, float("nan"))):
        y, ch = R.wsola(x[:L], t)
        assert np.array_equal(y, x[:L].astype(np.float64)) and len(ch) == 0


def test_wsola_test_inputs_have_the_properties_the_gpu_tests_rely_on():
    """unique cases: in every segment the fp64 maximum beats the runner-up by more than the recorded margin (so the device's fp32
    arg-max must equal the fp64 one); the zero-stretch case has segments whose dot products all tie; the shapes are the ones
    named in wsola_cases."""
    margin = noise()["wsola_dot_margin"]
    assert 0 < margin < 1e-3
    cases = {name: (x, tempo, unique) for name, x, tempo, unique in R.wsola_cases()}
    assert [R.segments(len(cases[n][0]), cases[n][1]) for n in ("copied_1545", "one_segment", "two_segments", "three_segments_zero_reads")] == [0, 1, 2, 3]
    assert {float(np.float32(t)) for _, t, _ in cases.values()} >= {float(np.float32(0.85)), 1.0, float(np.float32(1.15))}
    x, t, _ = cases["three_segments_zero_reads"]
    assert R.start(2, t) < len(x) < R.start(2, t) + R.SEARCH + R.OVL                       # the clip ends inside the last window
    ties = 0
    for name, (x, tempo, unique) in cases.items():
        _, chosen = R.wsola(x, tempo)
        prev = 0
        for k in range(1, len(chosen)):
            d = np.sort(R.dots(x, prev, k, tempo))[::-1]
            if unique:
                assert d[0] - d[1] > 100 * margin, (name, k, d[0] - d[1])
            elif d[0] == d[-1]:
                ties += 1
                assert chosen[k] == 0
            prev = R.start(k, tempo) + int(chosen[k])
    assert ties >= 2
