"""The rules of ds2_confidence (include/ds2hip.h) restated in numpy: fp64 in the fixed orders, rounded once
to fp32.  Nothing here looks at the device code; tests/test_gpu_confidence.py compares the kernels with it and
tests/test_confidence_host.py checks the rules' stated consequences on it."""
import math

import numpy as np

KINDS = {"logits": 0, "probs": 1, "log_probs": 2}
MEASURES = ("label_prob", "max_prob", "entropy", "tsallis", "renyi")
f32, f64 = np.float32, np.float64


def wave_sum(v):
    """sum of a 1-D fp64 array in the kernel's order: 64 partial sums over the classes j, j + 64, ... in increasing order, then
    v[j] += v[j ^ o] for o = 32, ..., 1"""
    part = np.zeros(64, f64)
    for c0 in range(0, len(v), 64):
        blk = v[c0:c0 + 64]
        part[:len(blk)] = part[:len(blk)] + blk
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[idx ^ o]
    return part[0]


def lognorm(row):
    """lz of one frame of logits: m + log(sum exp(x - m)) in fp64, rounded once"""
    with np.errstate(all="ignore"):
        m = np.max(row)
        return f32(f64(m) + np.log(wave_sum(np.exp(row.astype(f64) - f64(m)))))


def frame_probs(row, kind):
    """p_t(c) of one frame as fp32 numbers (and lz)"""
    with np.errstate(all="ignore"):
        if kind == "probs":
            return row.astype(f32), f32(0)
        if kind == "log_probs":
            return np.exp(row.astype(f64)).astype(f32), f32(0)
        lz = lognorm(row)
        return np.exp(row.astype(f64) - f64(lz)).astype(f32), lz


def argmax_first(row):
    """the greedy decoder's scan: best = 0; a later class wins only if strictly greater (false for NaN on either side)"""
    best = 0
    for c in range(1, len(row)):
        if row[c] > row[best]:
            best = c
    return best


def clamp01(v):
    return f32(0.0 if v < 0 else 1.0 if v > 1 else v)


def frame_value(p, a, measure, alpha):
    """m_t from the frame's fp32 probabilities p and its arg-max a"""
    V = len(p)
    if measure in ("label_prob", "max_prob"):
        return f32(p[a])
    pd = p.astype(f64)
    with np.errstate(all="ignore"):
        if measure == "entropy":
            s = wave_sum(np.where(pd == 0, 0.0, pd * np.log(pd)))
            return clamp01(1.0 - (-s) / math.log(V))
        s = wave_sum(np.power(pd, alpha))
        if measure == "tsallis":
            return clamp01(1.0 - ((1.0 - s) / (alpha - 1.0)) / ((1.0 - math.pow(V, 1.0 - alpha)) / (alpha - 1.0)))
        return clamp01(1.0 - (np.log(s) / (1.0 - alpha)) / math.log(V))


def frame_pass(x, size, kind, measure, alpha):
    """(a [size] int, m [size] f32, p [size][C] f32) of one clip's valid frames"""
    a, m, ps = [], [], []
    for t in range(size):
        p, _ = frame_probs(x[t], kind)
        at = argmax_first(x[t])
        a.append(at)
        m.append(frame_value(p, at, measure, alpha))
        ps.append(p)
    C = x.shape[1]
    return np.array(a, np.int64), np.array(m, f32), (np.stack(ps) if ps else np.zeros((0, C), f32))


def aggregate(values, how):
    """mean / min / prod of fp32 values in order: fp64 accumulation, one rounding; min by `v < best`.  NaN without values."""
    if len(values) == 0:
        return f32(np.nan)
    if how == "mean":
        acc = f64(0)
        for v in values:
            acc = acc + f64(v)
        return f32(acc / f64(len(values)))
    if how == "prod":
        acc = f64(values[0])
        for v in values[1:]:
            acc = acc * f64(v)
        return f32(acc)
    best = f32(values[0])
    for v in values[1:]:
        if v < best:
            best = f32(v)
    return best


def forward_end(a, size, tok, off, i):
    l, e = tok[i], off[i]
    lim = min(size, off[i + 1]) if i + 1 < len(tok) else size
    while e + 1 < lim and a[e + 1] == l:
        e += 1
    return e


def spans(a, size, tok, off):
    """[(s_i, e_i)] by the two walks"""
    out = []
    for i in range(len(tok)):
        e = forward_end(a, size, tok, off, i)
        floor_t = forward_end(a, size, tok, off, i - 1) if i > 0 else -1
        s = off[i]
        while s - 1 >= 0 and s - 1 > floor_t and a[s - 1] == tok[i]:
            s -= 1
        out.append((s, e))
    return out


def word_runs(tok, space):
    """[(first, last)] token indices of the maximal runs of non-space tokens"""
    runs, first = [], None
    for i, l in enumerate(tok):
        if l == space:
            if first is not None:
                runs.append((first, i - 1))
                first = None
        elif first is None:
            first = i
    if first is not None:
        runs.append((first, len(tok) - 1))
    return runs


def hypothesis(x, size, kind, tok, off, space, measure="label_prob", alpha=1 / 3, agg="mean", wagg="min", frames=None):
    """One hypothesis of one clip.  x: [T'][C] fp32; returns a dict: valid, tok_start, tok_end, tok_conf, words [(first, last,
    start, end, conf)], utt_conf (NaN without words).  frames: a frame_pass result to share between hypotheses."""
    C = x.shape[1]
    tok, off = [int(v) for v in tok], [int(v) for v in off]
    if any(not 0 <= l < C for l in tok) or any(not 0 <= o < size for o in off):
        return dict(valid=False, tok_start=[], tok_end=[], tok_conf=[], words=[], utt_conf=f32(np.nan))
    a, m, p = frames if frames is not None else frame_pass(x, size, kind, measure, alpha)
    sp = spans(a, size, tok, off)
    conf = []
    for (s, e), l in zip(sp, tok):
        vals = [p[t, l] if measure == "label_prob" else m[t] for t in range(s, e + 1)]
        conf.append(aggregate(vals, agg))
    words = [(f, l, sp[f][0], sp[l][1], aggregate(conf[f:l + 1], wagg)) for f, l in word_runs(tok, space)]
    return dict(valid=True, tok_start=[s for s, _ in sp], tok_end=[e for _, e in sp], tok_conf=conf, words=words,
                utt_conf=aggregate([w[4] for w in words], wagg))
