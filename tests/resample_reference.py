"""The resampler's definition restated in numpy, independent of deepspeech.pytorch_amd.resample: the
parameters, the fp64 taps, the one-shot sum (any dtype: fp64 for the real taps, int64 for the integer-operand tests, where it is
exact), the streaming plan and a chunked restatement that keeps a carry as the device does.  Every sum runs over the taps in rising
j, one vectorised step per tap, so the one-shot and the chunked restatement add the same numbers in the same order."""
import math

import numpy as np

OUT_RATE = 16000
RATES = (8000, 11025, 22050, 24000, 32000, 44100, 48000)


def params(in_rate, zeros=24):
    """(U, D, W)"""
    g = math.gcd(int(in_rate), OUT_RATE)
    U, D = OUT_RATE // g, int(in_rate) // g
    W = zeros if D <= U else (zeros * D + U - 1) // U
    return U, D, W


def taps64(in_rate, zeros=24, rolloff=0.92, beta=9.0):
    """[U][2W] float64, every phase normalised to sum 1"""
    U, D, W = params(in_rate, zeros)
    c = min(1.0, U / D) * rolloff
    h = np.zeros((U, 2 * W))
    for p in range(U):
        t = (np.arange(2 * W) - W + 1) - p / U
        ok = np.abs(t) <= W
        arg = np.where(ok, 1.0 - (t / W) ** 2, 0.0)
        h[p] = np.where(ok, c * np.sinc(c * t) * np.i0(beta * np.sqrt(np.maximum(arg, 0.0))) / np.i0(beta), 0.0)
        h[p] /= h[p].sum()
    return h


def taps32(in_rate):
    return taps64(in_rate).astype(np.float32)


def integer_taps(U, W):
    """((31 p + 17 j) mod 17) - 8: integers in [-8, 8] that tell every (phase, tap) pair from its neighbours"""
    p, j = np.arange(U, dtype=np.int64)[:, None], np.arange(2 * W, dtype=np.int64)[None, :]
    return ((31 * p + 17 * j) % 17) - 8


def out_len(n, U, D):
    return (int(n) * U + D - 1) // D


def resample(x, h, U, D, W, ms=None, first=0, end=None, magnitude=False):
    """y[m] = sum_j h[p][j] x[n0 - W + 1 + j] for the outputs `ms` (None = all out_len(len(x))) in the dtype of h.  x holds the
    clip positions [first, first + len(x)); positions outside [0, end) (end None = first + len(x)) read as zero.  magnitude: the
    sums of |h x| instead (the operand of the rounding bound)."""
    x = np.asarray(x)
    h = np.asarray(h)
    end = first + len(x) if end is None else end
    ms = np.arange(out_len(end, U, D), dtype=np.int64) if ms is None else np.asarray(ms, dtype=np.int64)
    n0, p = (ms * D) // U, (ms * D) % U
    xp = np.concatenate([np.zeros(2 * W, x.dtype), x, np.zeros(2 * W, x.dtype)]).astype(h.dtype)
    base = n0 - W + 1 - first + 2 * W
    y = np.zeros(len(ms), h.dtype)
    for j in range(2 * W):
        pos = base + j
        inside = (pos >= 0) & (pos < len(xp))
        term = h[p, j] * np.where(inside, xp[np.clip(pos, 0, len(xp) - 1)], 0)
        y += np.abs(term) if magnitude else term
    return y


def outputs_after(G, final, U, D, W):
    """E(G): the outputs that exist after G samples"""
    if final:
        return out_len(G, U, D)
    return 0 if G <= W else ((G - W) * U + D - 1) // D


def first_input(m, U, D, W):
    return max(0, (m * D) // U - W + 1)


def plan(G, n_new, final, U, D, W):
    """(out_before, emit, carried, new_carry, first) as the definition gives them"""
    e0, e1 = outputs_after(G, False, U, D, W), outputs_after(G + n_new, final, U, D, W)
    f0 = first_input(e0, U, D, W)
    return e0, e1 - e0, G - f0, 0 if final else G + n_new - first_input(e1, U, D, W), f0


class ChunkedResampler:
    """One stream fed in chunks: keeps the input samples the plan says to keep and nothing else."""

    def __init__(self, h, U, D, W):
        self.h, self.U, self.D, self.W = h, U, D, W
        self.G, self.carry, self.max_carry = 0, np.zeros(0, h.dtype), 0

    def feed(self, chunk, final=False):
        U, D, W = self.U, self.D, self.W
        e0, emit, carried, new_carry, f0 = plan(self.G, len(chunk), final, U, D, W)
        assert carried == len(self.carry), (carried, len(self.carry))
        win = np.concatenate([self.carry, np.asarray(chunk).astype(self.h.dtype)])
        G1 = self.G + len(chunk)
        y = resample(win, self.h, U, D, W, ms=np.arange(e0, e0 + emit, dtype=np.int64), first=f0, end=G1)
        self.carry = win[len(win) - new_carry:] if new_carry else np.zeros(0, self.h.dtype)
        self.G, self.max_carry = G1, max(self.max_carry, new_carry)
        return y


def prototype_response_db(h, in_rate, nfft=1 << 22):
    """(frequencies in Hz, 20 log10 |H(f)| / U) of the filter the table samples at U * in_rate: the taps of all phases interleaved
    (prototype index (j - W + 1) U - p), evaluated by a zero-padded fp64 FFT.  The passband gain of the table is U."""
    h = np.asarray(h, dtype=np.float64)
    U = h.shape[0]
    g = h[::-1].T.reshape(-1)
    H = np.abs(np.fft.rfft(g, nfft)) / U
    f = np.arange(len(H)) * (U * in_rate / nfft)
    return f, 20 * np.log10(np.maximum(H, 1e-300))
