"""Host checks of the resampler (deepspeech/pytorch_amd/resample.py, the host-only queries of
csrc/ds2_resample.hip): the filter the table samples, the closed-form streaming plan against the library's and against the
definition restated in tests/resample_reference.py, and the refusals.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import resample_reference as RR
from deepspeech.pytorch_amd import _lib
from deepspeech.pytorch_amd.resample import ResamplePlan, Resampler

SHAPES = {8000: (2, 1, 24), 11025: (640, 441, 24), 44100: (160, 441, 67), 48000: (1, 3, 72)}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("rate", RR.RATES)
def test_filter_response(rate):
    """the table's prototype in fp64: ripple over [0, 0.8 f_N] <= 0.01 dB, <= -90 dB from 1.08 f_N up (measured: at most 0.0004 dB and
    -91.9 dB); every fp32 phase sums to 1 within 1e-6; the table is the restatement's, rounded once"""
    rs = Resampler(rate)
    assert rs.taps.dtype == np.float32 and rs.taps.shape == (rs.up, 2 * rs.half_width)
    assert (rs.up, rs.down, rs.half_width) == RR.params(rate)
    assert np.array_equal(rs.taps, RR.taps32(rate))
    f, db = RR.prototype_response_db(rs.taps, rate)
    fn = min(rate, 16000) / 2.0
    ripple = float(np.abs(db[f <= 0.8 * fn]).max())
    stop = float(db[f >= 1.08 * fn].max())
    at_fn = float(db[np.argmin(np.abs(f - fn))])
    sums = rs.taps.astype(np.float64).sum(1)
    l1 = float(np.abs(rs.taps.astype(np.float64)).sum(1).max())
    print("%d Hz: ripple %.5f dB, stopband %.1f dB, at f_N %.1f dB, sum |h| <= %.3f" % (rate, ripple, stop, at_fn, l1))
    assert ripple <= 0.01 and stop <= -90.0
    assert np.abs(sums - 1.0).max() <= 1e-6
    assert l1 <= 2.2


@pytest.mark.parametrize("rate", sorted(SHAPES))
def test_shapes(rate):
    rs = Resampler(rate)
    assert (rs.up, rs.down, rs.half_width) == SHAPES[rate]
    assert rs.up * 2 * rs.half_width * 4 <= 128 * 1024
    for n in (0, 1, 2, 159, 160, 44100, 13_700_000):
        assert rs.out_len(n) == RR.out_len(n, rs.up, rs.down) == -(-n * 16000 // rate)


def test_sixteen_khz_is_the_identity():
    rs = Resampler(16000)
    assert rs.identity and (rs.up, rs.down) == (1, 1) and rs.out_len(777) == 777
    assert rs.plan_resample(100, 50, False)[:2] == (100, 50) and rs.plan_resample(100, 50, True).new_carry == 0


def lib_plan(lib, G, n, final, U, D, W):
    out = (C.c_long * 5)()
    assert lib.ds2_resample_plan(G, n, int(final), U, D, W, out) == 0
    return ResamplePlan(*[int(v) for v in out])


@pytest.mark.parametrize("rate", RR.RATES)
def test_plan_equals_the_library_and_the_definition(lib, rate):
    rs = Resampler(rate)
    U, D, W = rs.up, rs.down, rs.half_width
    rng = np.random.RandomState(rate)
    cases = [(0, 0, False), (0, 0, True), (0, 1, True), (W, 0, False), (W, 1, False), (W + 1, 0, True), (2 * W, 2 * W, False)]
    for _ in range(300):
        base = int(rng.choice([0, W, 3 * W, 10 ** 6, 2 ** 31, 2 ** 40]))
        cases.append((base + int(rng.randint(0, 4 * W + 7)), int(rng.choice([0, 1, W - 1, W, W + 1, 97, 4410, 2 ** 31 - 1])), bool(rng.randint(2))))
    for G, n, final in cases:
        mine = rs.plan_resample(G, n, final)
        assert mine == lib_plan(lib, G, n, final, U, D, W) == ResamplePlan(*RR.plan(G, n, final, U, D, W)), (G, n, final)
        assert 0 <= mine.carried <= 2 * W - 1 and 0 <= mine.new_carry <= 2 * W - 1 and mine.emit >= 0
        assert mine.first + mine.carried == G
        if not final and mine.emit:                                     # exactly the outputs whose last tap n0 + W has arrived
            last = mine.out_before + mine.emit - 1
            assert (last * D) // U + W <= G + n - 1 < ((last + 1) * D) // U + W


@pytest.mark.parametrize("rate", [8000, 11025, 24000, 44100, 48000])
def test_random_feed_schedules_telescope_and_equal_the_one_shot_restatement(rate):
    """fp64 throughout: chunks of random lengths, empty feeds among them, the end sometimes as a flush from no new samples"""
    rs = Resampler(rate)
    U, D, W = rs.up, rs.down, rs.half_width
    h = RR.taps32(rate).astype(np.float64)
    rng = np.random.RandomState(rate + 1)
    for trial in range(6):
        n = int(rng.choice([1, W, W + 1, 2 * W, 6 * W + 5, 1000 + rng.randint(0, 2000)]))
        x = rng.standard_normal(n)
        want = RR.resample(x, h, U, D, W)
        assert len(want) == rs.out_len(n)
        ref, got, pos, G, emitted = RR.ChunkedResampler(h, U, D, W), [], 0, 0, 0
        flush = bool(trial % 2)
        while True:
            c = min(n - pos, int(rng.choice([0, 1, W - 1, W, W + 1, 2 * W, 97, 3 * W + rng.randint(0, 50)])))
            final = pos + c == n and not flush
            p = rs.plan_resample(G, c, final)
            got.append(ref.feed(x[pos:pos + c], final))
            assert len(got[-1]) == p.emit and p.out_before == emitted and p.new_carry == len(ref.carry) <= 2 * W - 1
            pos, G, emitted = pos + c, G + c, emitted + p.emit
            if final:
                break
            if pos == n and flush and rng.randint(2):
                p = rs.plan_resample(G, 0, True)
                got.append(ref.feed(x[:0], True))
                emitted += p.emit
                assert len(got[-1]) == p.emit
                break
        assert emitted == rs.out_len(n)                                 # the emitted counts telescope
        assert np.array_equal(np.concatenate(got), want), (rate, n)
        assert ref.max_carry <= 2 * W - 1


def test_refusals(lib):
    for bad in (0, -8000, 44100.5):
        with pytest.raises(ValueError, match="positive integer"):
            Resampler(bad)
    with pytest.raises(ValueError, match=r"U = 16000.*D = 16001.*bytes"):
        Resampler(16001)                                                # 16000 phases of 50 taps: 3.2 MB
    with pytest.raises(ValueError, match="out_rate"):
        Resampler(48000, out_rate=8000)
    with pytest.raises(ValueError, match="samples_before"):
        Resampler(8000).plan_resample(-1, 0)
    st = Resampler(44100).stream(3, "cpu")                              # the host side of a stream: nothing is allocated before a feed
    chunk = torch.zeros((1, 8))
    with pytest.raises(ValueError, match="slots must be distinct"):
        st.feed([3], chunk, [8])
    with pytest.raises(ValueError, match="slots must be distinct"):
        st.feed([1, 1], torch.zeros((2, 8)), [8, 8])
    with pytest.raises(ValueError, match="not in this feed"):
        st.feed([0], chunk, [8], final=[1])
    with pytest.raises(ValueError, match="sample counts"):
        st.feed([0], chunk, [9])
    with pytest.raises(ValueError, match="not a slot"):
        st.reset([3])
    st.ended[2] = True                                                  # as a final feed leaves it
    with pytest.raises(ValueError, match="ended"):
        st.feed([2], chunk, [8])
    st.reset([2])
    with pytest.raises(_lib.Ds2HipError, match="no CPU path"):
        st.feed([2], chunk, [8])
    assert st.samples == [0, 0, 0]                                      # a refused feed moves nothing
    # the C entries refuse before they launch: no device is needed to be told so
    out = (C.c_long * 5)()
    assert lib.ds2_resample_plan(-1, 0, 0, 2, 1, 24, out) == 1002 and lib.ds2_resample_plan(0, 0, 0, 16000, 16001, 25, out) == 1002
    assert lib.ds2_resample(None, 8, None, 1, None, 2, 1, 24, None, 8, None, None) == 1002
    assert lib.ds2_resample_stream_feed(None, 0, None, 1, 0, 0, 1, None, 2, 1, 24, None, None, 0, None, None) == 1002


def test_host_only_queries(lib):
    assert lib.ds2_resample_out_len(44100, 160, 441) == 16000 and lib.ds2_resample_out_len(1, 1, 3) == 1
    assert lib.ds2_resample_out_len(0, 2, 1) == 0 and lib.ds2_resample_out_len(-1, 2, 1) == -1
    assert lib_plan(lib, 0, 100, True, 1, 3, 72) == ResamplePlan(0, 34, 0, 0, 0)
    assert lib.ds2_resample_stream_state_bytes(4, 67) == 4 * 134 * 4 and lib.ds2_resample_stream_ws_bytes(3, 24) == 3 * 48 * 4
    for rate, (U, D, W) in SHAPES.items():
        tile = lib.ds2_resample_tile(U, D, W)
        assert tile >= 64 and tile % U == 0                             # whole periods of the phase sequence
    assert lib.ds2_resample_tile(16000, 16001, 25) == -1
