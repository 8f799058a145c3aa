"""Plain-Python restatements of the endpointing rule and the planted inputs that the endpoint tests
share.  Nothing here needs a GPU.

A frame is SILENT iff its blank probability, as fp32, is > the threshold as fp32 (strict; a NaN is not silent).  A segment starts
at frame s (0, or one past the previous endpoint); walking t = s, s + 1, ... with trailing = the consecutive silent frames ending
at t and spoken = some frame of [s, t] was not silent, it ends at the first t where, in this order,
    "silence": spoken and trailing >= min_trailing      "leading": not spoken and trailing >= max_leading
    "length":  t - s + 1 == max_segment
holds.  What is left open when the stream ends closes with reason "final" (possibly empty: end = start - 1)."""
import numpy as np

REASONS = (None, "silence", "leading", "length", "final")


def silent_mask(blank_probs, threshold):
    """the silent predicate as the device evaluates it: an fp32 compare, strict"""
    return np.asarray(blank_probs, np.float32) > np.float32(threshold)


class Walker:
    """The rule one frame at a time: the state that ds2_endpoint_feed keeps per stream."""

    def __init__(self, min_trailing, max_leading, max_segment):
        self.min_trailing, self.max_leading, self.max_segment = min_trailing, max_leading, max_segment
        self.start, self.trailing, self.spoken, self.consumed, self.segments = 0, 0, 0, 0, 0

    def state(self):
        return [self.start, self.trailing, self.spoken, self.consumed, self.segments]

    def step(self, silent):
        """consumes one frame; returns None or the event (reason, start, end, index) of the segment that ends on it"""
        t = self.consumed
        self.consumed += 1
        self.trailing = self.trailing + 1 if silent else 0
        self.spoken = int(self.spoken or not silent)
        reason = None
        if self.spoken and self.trailing >= self.min_trailing:
            reason = "silence"
        elif not self.spoken and self.trailing >= self.max_leading:
            reason = "leading"
        elif t - self.start + 1 == self.max_segment:
            reason = "length"
        if reason is None:
            return None
        ev = (reason, self.start, t, self.segments)
        self.start, self.trailing, self.spoken, self.segments = t + 1, 0, 0, self.segments + 1
        return ev

    def feed(self, silent):
        """ds2_endpoint_feed on one stream's part of a chunk: stops at the first endpoint.  Returns (cut, rest, event or None)."""
        for i, s in enumerate(silent):
            ev = self.step(bool(s))
            if ev is not None:
                return i + 1, len(silent) - i - 1, ev
        return len(silent), 0, None

    def close(self):
        ev = ("final", self.start, self.consumed - 1, self.segments)
        self.start, self.trailing, self.spoken, self.segments = self.consumed, 0, 0, self.segments + 1
        return ev


def segments_walk(silent, min_trailing, max_leading, max_segment, final=True):
    """[(start, end, reason)] of a whole stream, by the walk"""
    w = Walker(min_trailing, max_leading, max_segment)
    out = [ev[1:3] + ev[:1] for ev in (w.step(bool(s)) for s in silent) if ev is not None]
    if final:
        ev = w.close()
        out.append((ev[1], ev[2], ev[0]))
    return out


def segments_enumerate(silent, min_trailing, max_leading, max_segment, final=True):
    """The same list from a second formulation: per segment, the candidate end of each reason is computed on its own from the
    positions of the non-silent frames, and the earliest wins (ties in the order silence, leading, length)."""
    silent = np.asarray(silent, bool)
    T = len(silent)
    loud = np.flatnonzero(~silent)
    out, s = [], 0
    while s < T:
        after = loud[loud >= s]
        first = int(after[0]) if len(after) else T                 # the first non-silent frame of the segment
        cand = []
        # silence: the first window of min_trailing silent frames that begins after a non-silent frame at or after `first`
        for q in after:
            nxt = after[after > q]
            run_end = int(nxt[0]) if len(nxt) else T                # the silent run is (q, run_end)
            if run_end - q - 1 >= min_trailing:
                cand.append((int(q) + min_trailing, 0, "silence"))
                break
        if first - s >= max_leading:
            cand.append((s + max_leading - 1, 1, "leading"))
        cand.append((s + max_segment - 1, 2, "length"))
        end, _, reason = min(c for c in cand)
        if end >= T:
            break
        out.append((s, end, reason))
        s = end + 1
    if final:
        out.append((s, T - 1, "final"))
    return out


def sub_feeds(size, limit):
    """the sub-feed sizes of one stream's chunk of `size` frames under the limit (decoder.split_feed for one stream)"""
    return [min(limit, size - t0) for t0 in range(0, size, limit)]


# ---- planted inputs ---------------------------------------------------------------------------------------------------------------
# schedule letters: S speech (blank probability low), b silent, e blank probability == threshold (not silent), a the next fp32
# above the threshold (silent)
MIN_TRAILING, MAX_LEADING, MAX_SEGMENT, THRESHOLD = 3, 5, 12, 0.8
SCHEDULES = (
    # 0-4 leading silence of max_leading -> "leading" at 4 | a run of min_trailing - 1 (no cut) then one of min_trailing -> 13 |
    # 33 frames of speech: "length" at 25 and 37 | "silence" and "length" both due at 49 | blank == threshold is not silent, the
    # next float above it is: "silence" at 56 | leading silence of max_leading - 1 is no cut: "silence" at 65 | 4 frames left open
    "bbbbb" + "SSbbSSbbb" + "S" * 33 + "bbb" + "Seeeaaa" + "bbbbSSbbb" + "SSSS",
    # "silence" at 5 | max_leading - 1 leading, then speech: 14 | "leading" at 19 | then runs of every short length
    "SSSbbb" + "bbbbSSbbb" + "bbbbb" + "SbSbbSSbbbSSSSbbbbSbbSSSSSSSSSSSSbbbSbSSb",
    "SbbSSSbbbbbbbbSSSSSbbSbbbSSSSSSSSSSSSSbbbbbbSSbSSbbbSSSSSbbbbbbbbbSS",
)
TOTALS = tuple(len(s) for s in SCHEDULES)
assert TOTALS == (70, 61, 68)


def planted_probs(C, seed, schedules=SCHEDULES, threshold=THRESHOLD, path=None, blank=0):
    """(N, max T, C) fp32 probabilities that follow the schedules: the blank probability of every frame is set exactly, the rest
    of the mass is a peaky softmax over the other classes (peak on path[n][i] for the i-th speech frame of stream n when a path
    is given).  Frames past a stream's schedule are NaN."""
    rng = np.random.default_rng(seed)
    thr = np.float32(threshold)
    p = np.full((len(schedules), max(len(s) for s in schedules), C), np.nan, np.float32)
    others = [c for c in range(C) if c != blank]
    for n, sched in enumerate(schedules):
        k = 0
        for t, ch in enumerate(sched):
            z = rng.standard_normal(C - 1) * 1.5
            if ch in "Se":
                lab = path[n][k % len(path[n])] if path is not None else others[int(rng.integers(0, C - 1))]
                z[others.index(lab)] += 4.0
                k += 1
            pb = {"S": np.float32(rng.uniform(0.02, 0.3)), "b": np.float32(rng.uniform(0.85, 0.99)), "e": thr,
                  "a": np.nextafter(thr, np.float32(1))}[ch]
            e = np.exp(z - z.max())
            p[n, t, others] = (e / e.sum() * (1.0 - float(pb))).astype(np.float32)
            p[n, t, blank] = pb
    return p


def planted_silent(schedules=SCHEDULES):
    return [np.array([ch in "ba" for ch in s]) for s in schedules]
