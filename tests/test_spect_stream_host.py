"""Host checks of the streaming front-end's sample plan (spectrogram.plan_wave == ds2_spect_stream_plan) and of the fp64
restatement of the running normalisation (tests/spect_stream_reference.py).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import spect_stream_reference as SR
from spect_stream_reference import HOP, NFFT

LENGTHS = [1, 159, 160, 161, 319, 320, 321, 479, 480, 2037]
CHUNKS = [1, 7, 159, 160, 161, 319, 333, None]                     # None = the whole clip in one feed
NAMES = ["ds2_spect_running_ws_bytes", "ds2_spectrogram_running", "ds2_spect_stream_plan", "ds2_spect_stream_state_bytes",
         "ds2_spect_stream_ws_bytes", "ds2_spect_stream_feed"]


def cases():
    return [(L, c) for L in LENGTHS for c in CHUNKS if c != 1 or L <= 321]


@pytest.fixture(scope="module")
def lib():
    from deepspeech.pytorch_amd import _lib
    return _lib.load()


def c_plan(lib, G0, n, final):
    out = (C.c_int * 6)()
    assert lib.ds2_spect_stream_plan(G0, n, int(final), out) == 0
    return tuple(out)


@pytest.mark.parametrize("flush_only", [False, True])
@pytest.mark.parametrize("L,chunk", cases())
def test_plan_tiles_the_padded_clip(lib, L, chunk, flush_only):
    """Over a clip's feeds: the emitted counts sum to 1 + L // 160, the carry never exceeds 319, every emitted frame's 320
    samples stand in the feed's window where the padded clip has them, the windows' consumed parts concatenated are the padded
    clip, and the Python plan, the C plan and the restatement agree."""
    from deepspeech.pytorch_amd.spectrogram import plan_wave
    x = np.random.RandomState(L).standard_normal(L)
    P = SR.padded(x)
    carry, G, emitted, pieces = np.zeros(HOP), 0, 0, []
    for n, final in SR.feeds_of(L, chunk, final_with_samples=not flush_only):
        p = plan_wave(G, n, final)
        assert tuple(p) == c_plan(lib, G, n, final) == SR.sample_plan(G, n, final), (G, n, final)
        assert p.frames_before == emitted and p.carried == len(carry) and p.first == HOP * emitted - HOP
        window = np.concatenate([carry, x[G:G + n], np.zeros(HOP if final else 0)])
        assert len(window) == p.window and HOP * p.emit + (HOP if p.emit else 0) <= p.window
        for j in range(p.emit):
            assert np.array_equal(window[HOP * j:HOP * j + NFFT], P[HOP * (emitted + j):HOP * (emitted + j) + NFFT])
        pieces.append(window[:HOP * p.emit])
        carry = window[HOP * p.emit:]
        assert final or (len(carry) == p.new_carry and HOP <= len(carry) <= NFFT - 1)
        G, emitted = G + n, emitted + p.emit
    assert final and p.new_carry == 0 and p.emit >= 1                # the final feed always completes a frame
    assert G == L and emitted == 1 + L // HOP
    assert np.array_equal(np.concatenate(pieces + [carry]), P)


def test_plan_refuses_negative_and_null(lib):
    from deepspeech.pytorch_amd.spectrogram import plan_wave
    out = (C.c_int * 6)()
    assert lib.ds2_spect_stream_plan(-1, 1, 0, out) != 0 and lib.ds2_spect_stream_plan(0, -1, 0, out) != 0
    assert lib.ds2_spect_stream_plan(0, 1, 0, None) != 0
    for bad in ((-1, 1), (0, -1)):
        with pytest.raises(ValueError):
            plan_wave(*bad)


def test_sizes(lib):
    for S in (1, 3, 64):
        assert lib.ds2_spect_stream_state_bytes(S) == S * (16 + 320 * 4)
    assert lib.ds2_spect_stream_state_bytes(0) == 0 and lib.ds2_spect_stream_ws_bytes(0, 1, 1) == -1
    for N, L in ((1, 159), (3, 10240)):
        T = 1 + L // HOP
        assert lib.ds2_spect_running_ws_bytes(N, L) == lib.ds2_spect_ws_bytes(N, L) + N * T * 24
    for n, mx, Tc in ((1, 0, 0), (3, 480, 4), (2, 2037, 13)):
        lw = (mx + 2 * NFFT + 3) // 4 * 4 + NFFT
        assert lib.ds2_spect_stream_ws_bytes(n, mx, Tc) == ((n * lw + n * Tc * 336 + 2 * n * Tc) * 4 + 15) // 16 * 16 + 2 * n * Tc * 8


def test_exports_are_declared_bound_and_sized(lib):
    from deepspeech.pytorch_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ds2hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"^(?:int|long) %s\(([^;]*)\);" % name, hdr, re.M)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    body = re.search(r"typedef struct ds2_spect_stream_row \{(.*?)\} ds2_spect_stream_row;", hdr, re.S).group(1)
    from deepspeech.pytorch_amd.spectrogram import SPECT_ROW_WORDS
    assert len(re.findall(r"int32_t\s+\w+;", body)) == SPECT_ROW_WORDS == 8


def test_running_restatement_is_the_definition():
    """frame t against a direct evaluation over all values of frames 0..t; the floor on silence; the prior as pseudo-counts."""
    rs = np.random.RandomState(3)
    v = np.abs(rs.standard_normal((161, 9))) + 0.3
    y = SR.running_normalize(v)
    for t in range(9):
        head = v[:, :t + 1]
        assert np.allclose(y[:, t], (v[:, t] - head.mean()) / head.std(ddof=1), rtol=1e-10, atol=1e-12)
    z = np.zeros((161, 4))
    assert np.all(SR.running_normalize(z) == 0) and np.all(np.isfinite(SR.running_normalize(z)))
    mean, rstd = SR.running_stats(z, floor=1e-3)
    assert np.all(rstd == 1e3)
    # a prior of k frames = k frames whose values have exactly that mean and (population) standard deviation, in front
    k, pm, ps = 3, 0.8, 0.5
    fake = np.tile(np.concatenate([np.full(80, pm - ps), np.full(80, pm + ps), [pm]])[:, None], (1, k))
    pop_std = np.sqrt(((fake - pm) ** 2).mean())
    want = SR.running_normalize(np.concatenate([fake, v], 1))[:, k:]
    got = SR.running_normalize(v, prior=(pm, pop_std, k))
    assert np.allclose(got, want, rtol=1e-9, atol=1e-11)


def test_front_end_arguments():
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    assert SpectrogramFrontEnd().normalize is True and SpectrogramFrontEnd(normalize=False).normalize is False
    fe = SpectrogramFrontEnd(normalize="running", running_prior=(0.5, 0.4, 20))
    assert fe.normalize == "running" and fe.running and fe.running_floor == 1e-5 and fe.running_prior == (0.5, 0.4, 20.0)
    for kw in (dict(normalize="causal"), dict(normalize="running", running_floor=0.0), dict(normalize="running", running_prior=(0, -1, 2)),
               dict(normalize="running", running_prior=(0, 1))):
        with pytest.raises(ValueError):
            SpectrogramFrontEnd(**kw)
