"""fp64 numpy restatement of the reverberation rules (DESIGN.md section 7.1 "Reverberation"; the reference has no reverberation,
so there is no golden fixture): the convolution of ds2_reverb, the bank rules of augment.RirBank, and the per-clip draw order of
augment.WaveAugment.draw with a rir_bank.  Nothing here imports the package."""
import math

import numpy as np


def reverb_ref(x, L, h, p, ldo):
    """out[i] = sum_k h[k] x[i + p - k] for i < L, x = 0 outside [0, L); zero from L to ldo.  fp64 (int64 for integer inputs)."""
    x, h = np.asarray(x), np.asarray(h)
    wide = np.int64 if np.issubdtype(x.dtype, np.integer) and np.issubdtype(h.dtype, np.integer) else np.float64
    out = np.zeros(ldo, wide)
    full = np.convolve(x[:L].astype(wide), h.astype(wide))          # full[j] = sum_k h[k] x[j - k], j in [0, L + K - 1)
    n = min(L, ldo)
    seg = full[p:p + n]
    out[:len(seg)] = seg
    return out


def reverb_abs_ref(x, L, h, p, ldo):
    """sum_k |h[k]| |x[i + p - k]|: what the rounding bound of the float test scales with."""
    return reverb_ref(np.abs(np.asarray(x, np.float64)), L, np.abs(np.asarray(h, np.float64)), p, ldo)


def prepare_ref(h, normalize="energy", max_taps=16384):
    """RirBank's rules for one response -> (fp32 taps, peak index); raises ValueError where the bank refuses."""
    h = np.asarray(h, np.float64).reshape(-1)
    if h.size == 0 or not np.any(h != 0):
        raise ValueError("empty or all-zero")
    a = np.abs(h)
    p = next(i for i in range(len(a)) if a[i] == a.max())            # the FIRST arg-max
    if p >= max_taps:
        raise ValueError("peak beyond max_taps")
    h = h[:max_taps]
    if normalize == "energy":
        h = h / math.sqrt(float((h * h).sum()))
    elif normalize == "peak":
        h = h / abs(float(h[p]))
    elif normalize is not None:
        raise ValueError(normalize)
    return h.astype(np.float32), p


def synthetic_ref(rt60, rng, drr_db=0.0, sample_rate=16000):
    """h[0] = 1, h[k] = a g_k exp(-3 ln10 k / (rt60 sample_rate)), sum_{k > 0} h^2 = 10^(-drr_db / 10); ceil(rt60 sample_rate) taps."""
    n = int(math.ceil(rt60 * sample_rate))
    h = np.zeros(n)
    h[0] = 1.0
    if n > 1:
        g = rng.standard_normal(n - 1)
        tail = g * np.exp(-3.0 * math.log(10.0) * np.arange(1, n) / (rt60 * sample_rate))
        h[1:] = tail * math.sqrt(10.0 ** (-drr_db / 10.0) / float((tail * tail).sum()))
    return h


class FakeBank:
    """what draw() asks of a NoiseBank or a RirBank, without a device."""

    def __init__(self, lengths, peaks=None):
        self.offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        self.peaks = np.zeros(len(lengths), np.int32) if peaks is None else np.asarray(peaks, np.int32)

    def __len__(self):
        return len(self.offsets) - 1

    def length(self, r):
        return int(self.offsets[r + 1] - self.offsets[r])


def draw_ref(nsamples, rng, speed_volume_perturb=False, tempo_range=(0.85, 1.15), gain_range=(-6, 8), noise_bank=None,
             noise_prob=0.4, noise_levels=(0.0, 0.5), rir_bank=None, rir_prob=0.5, out_len=None):
    """The per-clip draw order with reverberation: tempo, gain, [binomial(rir_prob), choice(len(rir_bank))], binomial(noise_prob),
    choice, level, rand.  out_len(L, tempo) = the length after the tempo change.  Returns a dict of lists, one entry per clip (None
    where the step is off)."""
    res = dict(tempo=[], gain_db=[], rir=[], noise=[], nsamples=[])
    for L in nsamples:
        L = int(L)
        tempo = gain_db = None
        if speed_volume_perturb:
            tempo = float("%.3f" % rng.uniform(low=tempo_range[0], high=tempo_range[1]))
            gain_db = float("%.3f" % rng.uniform(low=gain_range[0], high=gain_range[1]))
            L = out_len(L, tempo)
        rir = None
        if rir_bank is not None:
            rir = -1
            if rng.binomial(1, rir_prob):
                rir = int(rng.choice(len(rir_bank)))
        noise = None
        if noise_bank is not None:
            noise = (-1, 0.0, 0)
            if rng.binomial(1, noise_prob):
                r = int(rng.choice(len(noise_bank)))
                lv = rng.uniform(*noise_levels)
                u = rng.random()
                nl = noise_bank.length(r)
                if L <= nl:
                    start = min(max(int(u * (nl / 16000.0 - L / 16000.0) * 16000.0), 0), nl - L)
                    noise = (int(noise_bank.offsets[r]), lv, start)
        for k, v in (("tempo", tempo), ("gain_db", gain_db), ("rir", rir), ("noise", noise), ("nsamples", L)):
            res[k].append(v)
    return res
