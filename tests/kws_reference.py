"""The keyword-spotting rule of include/ds2hip.h restated in float32 numpy, in the stated order.

``RefStream`` is one stream: ``feed(x, end=False)`` takes a (T, C) array of class scores (what `kind` says) and returns the hits
that this feed emits, as the device lists them: (keyword, start, end, score) in (keyword, time) order, at most max_hits per
keyword, the others counted in ``dropped``.  ``best`` is [(score, start, end)] per keyword.  Nothing here knows about waves,
lanes or chunks of frames: a keyword is an array of 2L - 1 states that is walked frame by frame."""
import numpy as np

F32 = np.float32
NINF = F32(-np.inf)


def frame_scores(x, kind):
    """r[t][c] = lp[t][c] - max_c' lp[t][c'], fp32; lp = x for "logits" and "log_probs", log(x) for "probs" """
    x = np.asarray(x, F32)
    if kind == "probs":
        with np.errstate(divide="ignore"):
            lp = np.log(x).astype(F32)
    elif kind in ("logits", "log_probs"):
        lp = x
    else:
        raise ValueError(kind)
    return (lp - lp.max(axis=1, keepdims=True)).astype(F32) if x.shape[0] else lp


def threshold_abs(threshold, L):
    return F32(np.float64(threshold) * L)


class RefKeyword:
    """The lattice, the candidate and the best of one keyword in one stream."""

    def __init__(self, ids, blank, thr_abs):
        L = len(ids)
        assert 1 <= L <= 64 and blank not in ids
        self.ext = np.array([ids[s // 2] if s % 2 == 0 else blank for s in range(2 * L - 1)], np.int64)
        # s - 2 is allowed into a label state whose label differs from the label before it
        self.skip = np.array([s >= 2 and s % 2 == 0 and ids[s // 2] != ids[s // 2 - 1] for s in range(2 * L - 1)])
        self.thr = F32(thr_abs)
        self.v = np.full(2 * L - 1, NINF, F32)
        self.b = np.full(2 * L - 1, -1, np.int64)
        self.cand = None                           # (score, start, end) of the open candidate
        self.best = (NINF, -1, -1)

    def step(self, r, t):
        """one frame: r [C] frame scores, t the absolute frame; returns the end score (s_t, b_t)"""
        v, b = self.v, self.b
        best, bb = v.copy(), b.copy()
        # s - 1; for state 0 the fresh start (0, t) stands there: taken only when strictly greater
        c1 = np.concatenate([[F32(0)], v[:-1]]).astype(F32)
        b1 = np.concatenate([[t], b[:-1]])
        take = c1 > best
        best, bb = np.where(take, c1, best), np.where(take, b1, bb)
        if len(v) > 2:
            c2 = np.concatenate([[NINF, NINF], v[:-2]]).astype(F32)
            b2 = np.concatenate([[-1, -1], b[:-2]])
            take = self.skip & (c2 > best)
            best, bb = np.where(take, c2, best), np.where(take, b2, bb)
        self.v = (best.astype(F32) + r[self.ext].astype(F32)).astype(F32)
        self.b = np.where(self.v == NINF, -1, bb)
        return self.v[-1], int(self.b[-1])


class RefStream:
    def __init__(self, keyword_ids, thresholds, blank, hold=25, max_hits=8, kind="log_probs"):
        """keyword_ids: [[label ids]]; thresholds: nats per label, one per keyword"""
        self.kws = [RefKeyword(list(ids), blank, threshold_abs(th, len(ids))) for ids, th in zip(keyword_ids, thresholds)]
        self.hold, self.max_hits, self.kind = int(hold), int(max_hits), kind
        self.frames, self.dropped = 0, 0

    def feed(self, x, end=False):
        x = np.asarray(x, F32)
        r = frame_scores(x, self.kind) if x.shape[0] else x
        lists = [[] for _ in self.kws]
        for i in range(x.shape[0]):
            t = self.frames + i
            for k, kw in enumerate(self.kws):
                if kw.cand is not None and t - kw.cand[2] >= self.hold:                 # 1
                    lists[k].append(kw.cand)
                    kw.cand = None
                s, b = kw.step(r[i], t)
                if s >= kw.thr and s > NINF:                                             # 2
                    if kw.cand is None or s > kw.cand[0] or (s == kw.cand[0] and b == kw.cand[1]):
                        kw.cand = (s, b, t)
                if s > kw.best[0]:
                    kw.best = (s, b, t)
        self.frames += x.shape[0]
        if end:
            for k, kw in enumerate(self.kws):
                if kw.cand is not None:
                    lists[k].append(kw.cand)
                    kw.cand = None
        hits = []
        for k, l in enumerate(lists):
            hits += [(k, int(b), int(e), F32(s)) for s, b, e in l[:self.max_hits]]
            self.dropped += max(len(l) - self.max_hits, 0)
        return hits

    @property
    def best(self):
        return [(F32(kw.best[0]), int(kw.best[1]), int(kw.best[2])) for kw in self.kws]


def spot(x, keyword_ids, thresholds, blank, hold=25, max_hits=8, kind="log_probs"):
    """one clip, one shot: (hits, best, dropped)"""
    st = RefStream(keyword_ids, thresholds, blank, hold, max_hits, kind)
    hits = st.feed(x, end=True)
    return hits, st.best, st.dropped


def end_scores(x, ids, blank, kind="log_probs"):
    """s_t of one keyword for every frame of x"""
    r = frame_scores(x, kind)
    kw = RefKeyword(list(ids), blank, NINF)
    return np.array([kw.step(r[t], t)[0] for t in range(r.shape[0])], F32)


def by_time(hits):
    """the order the Python layer gives: (end_frame, keyword index)"""
    return sorted(hits, key=lambda h: (h[2], h[0]))


def grid_log_probs(rng, T, C, lo=-12.0):
    """scores that are multiples of 1/8 in [lo, 0]: every fp32 sum of them is exact (tests/test_gpu_ctc_align.py's device)"""
    return (rng.integers(int(lo * 8), 1, size=(T, C)) / 8.0).astype(F32)
