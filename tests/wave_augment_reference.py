"""Restatement in numpy fp64 of the waveform augmentations of csrc/ds2_waveaug.hip, written from the rules of DESIGN.md section 7
and not from the kernels' code path: one clip at a time, plain loops, fp64 throughout.

WSOLA (sox `tempo` defaults at 16 kHz: segment 1312, 234 candidate offsets, overlap 192; a segment advances the output by 1120):
    start(k) = floor(k * tempo * 1120)          tempo is an fp32 value, the product is fp64
    S        = number of k with start(k) + 192 <= L
    out_len  = (S - 1) * 1120 + min(1312, L - start(S - 1))
    p(0) = 0, p(k) = start(k) + d(k); d(k) = the lowest d in [0, 234) that maximises sum_j x[p(k-1) + 1120 + j] * x[start(k) + d + j]
    over j in [0, 192); x is zero at and beyond L
    out[1120 k + j] = x[p(k) + j]; for k >= 1 and j < 192 it is a + (j / 192) * (x[p(k) + j] - a) with a = x[p(k-1) + 1120 + j]
    the last segment runs to out_len
A clip with L < 1312 + 234 or a tempo outside [0.1, 10] is copied unchanged.

Gain: clamp(10^(dB / 20) * x, -1, 1) with the factor rounded to fp32 (the kernels take the fp32 factor, the product is one
correctly rounded fp32 multiply; no 16-bit requantisation, no dither).
Mix (loader/data_loader.py:125-127): y + level * noise * rms(y) / rms(noise), both over the clip's length; a noise crop without
energy, a level <= 0 or no noise leaves y."""
import math

import numpy as np

SEG, SEARCH, OVL = 1312, 234, 192
ADV = SEG - OVL


def start(k, tempo):
    return math.floor(k * float(np.float32(tempo)) * float(ADV))


def runs(L, tempo):
    t = np.float32(tempo)
    return bool(L >= SEG + SEARCH and np.float32(0.1) <= t <= np.float32(10.0))


def segments(L, tempo):
    if not runs(L, tempo):
        return 0
    k = 0
    while start(k + 1, tempo) + OVL <= L:
        k += 1
    return k + 1


def out_len(L, tempo):
    S = segments(L, tempo)
    if S == 0:
        return max(int(L), 0)
    return (S - 1) * ADV + min(SEG, L - start(S - 1, tempo))


def _read(x, a, n):
    """x[a : a + n] with zeros at and beyond len(x)."""
    out = np.zeros(n, np.float64)
    m = max(0, min(n, len(x) - a))
    out[:m] = x[a:a + m]
    return out


def dots(x, prev, k, tempo, dtype=np.float64):
    """the 234 dot products of segment k >= 1 given p(k - 1) = prev, evaluated in `dtype`."""
    x = np.asarray(x)
    tail = _read(x, prev + ADV, OVL).astype(dtype)
    win = _read(x, start(k, tempo), SEARCH + OVL).astype(dtype)
    return np.array([np.dot(tail, win[d:d + OVL]) for d in range(SEARCH)], dtype)


def wsola(x, tempo, offsets=None):
    """-> (out fp64 [out_len], chosen offsets [S] int).  offsets: force these instead of searching (entries of segments >= 1)."""
    x = np.asarray(x, np.float64)
    L, S = len(x), segments(len(x), tempo)
    if S == 0:
        return x.copy(), np.zeros(0, np.int64)
    n_out = out_len(L, tempo)
    out, chosen = np.zeros(n_out, np.float64), np.zeros(S, np.int64)
    prev = 0
    fade = np.arange(OVL, dtype=np.float64) / OVL
    for k in range(S):
        d = 0
        if k > 0:
            d = int(offsets[k]) if offsets is not None else int(np.argmax(dots(x, prev, k, tempo)))      # argmax: the first maximum
        chosen[k] = d
        p = start(k, tempo) + d
        n = ADV if k + 1 < S else min(SEG, L - start(k, tempo))
        seg = _read(x, p, n)
        if k > 0:
            a = _read(x, prev + ADV, OVL)
            seg[:OVL] = a + fade * (seg[:OVL] - a)
        out[k * ADV:k * ADV + n] = seg
        prev = p
    return out, chosen


def gain_factor(db):
    return np.float32(10.0 ** (float(db) / 20.0))


def gain(x, db):
    """fp32 in, fp32 out: exactly what one fp32 multiply and a clamp give."""
    return np.clip(gain_factor(db) * np.asarray(x, np.float32), np.float32(-1), np.float32(1)).astype(np.float32)


def energies(y, noise):
    y, noise = np.asarray(y, np.float64), np.asarray(noise, np.float64)
    return float(np.dot(y, y)), float(np.dot(noise, noise))


def scale(y, noise, level):
    ed, en = energies(y, noise)
    return float(level) * math.sqrt(ed / en) if (level > 0 and en > 0) else 0.0


def mix(y, noise, level):
    """y: the gained clip; noise: its crop (same length) or None."""
    y = np.asarray(y, np.float64)
    if noise is None:
        return y.copy()
    return y + scale(y, noise, level) * np.asarray(noise, np.float64)


# ---- the WSOLA inputs of the tests (shared by tests/golden/make_wave_augment.py, which measures the fp32 dot-product margin on
# them, and by the host and GPU tests) ----------------------------------------------------------------------------------------
def chirp_noise(L, seed, f0=300.0, f1=1500.0, amp=0.5, noise=0.05):
    """a chirp from f0 to f1 Hz over the clip (16 kHz) plus seeded white noise, fp32: the correlation peak of every segment is
    unique (the instantaneous frequency never repeats) and far from flat."""
    t = np.arange(L, dtype=np.float64) / 16000.0
    dur = max(L, 1) / 16000.0
    x = amp * np.sin(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) / dur * t * t))
    return (x + noise * np.random.RandomState(seed).standard_normal(L)).astype(np.float32)


def wsola_cases():
    """(name, x fp32, tempo, unique): `unique` = the fp64 maximum of every segment is meant to be unique by more than the recorded
    margin (asserted on the CPU by tests/test_wave_augment_host.py).  The first five form one batch (N = 5), the last runs alone."""
    zero = chirp_noise(12000, 5)
    zero[4000:7000] = 0.0                                  # tails inside the stretch are all zero: every dot product ties at 0
    return [("copied_1545", chirp_noise(SEG + SEARCH - 1, 1), 1.15, True),          # shorter than segment + search
            ("one_segment", chirp_noise(1800, 2), 1.5, True),                        # start(1) + 192 = 1872 > 1800
            ("two_segments", chirp_noise(1612, 3), 1.0, True),                       # start(1) = 1120, start(2) = 2240
            ("three_segments_zero_reads", chirp_noise(2300, 4), 0.85, True),         # start(2) = 1904: its window ends at 2330
            ("zero_stretch", zero, 1.15, False),
            ("alone_5000", chirp_noise(5000, 6), 1.0, True)]
