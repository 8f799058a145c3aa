"""fp64 numpy restatement of CTC forced alignment as include/ds2hip.h states it for ds2_ctc_align: the lattice, the tie rule, the
infeasible case and the per-label spans.  Written from the statement, not from the kernel: states are a numpy vector, the
predecessor choice is three comparisons in the order the tie rule gives.

    ext[2i] = blank, ext[2i+1] = target[i]                 S = 2L + 1 states
    v[0][0] = lp[0][blank], v[0][1] = lp[0][ext[1]], every other state -inf
    v[t][s] = lp[t][ext[s]] + max(v[t-1][s], v[t-1][s-1], v[t-1][s-2])       s-2 only for a label that differs from ext[s-2]
    ties: s, then s-1, then s-2; at the end an equal value goes to 2L rather than 2L - 1
"""
from collections import namedtuple

import numpy as np

Aligned = namedtuple("Aligned", "score frame_state tok_start tok_end tok_logp")


def extended(target, blank):
    ext = np.full(2 * len(target) + 1, blank, dtype=np.int64)
    ext[1::2] = target
    return ext


def align(lp, target, blank=0):
    """lp: [T][C] log-probabilities (float64, -inf allowed) of the clip's own frames; target: its labels.  Returns Aligned:
    score (-inf = no path: then frame_state, tok_start, tok_end are -1 and tok_logp 0), frame_state [T], tok_* [L]."""
    lp = np.asarray(lp, dtype=np.float64)
    target = np.asarray(target, dtype=np.int64).reshape(-1)
    T, L = lp.shape[0], len(target)
    none = Aligned(-np.inf, np.full(T, -1, np.int64), np.full(L, -1, np.int64), np.full(L, -1, np.int64), np.zeros(L))
    if T == 0:
        return none
    ext = extended(target, blank)
    S = len(ext)
    skip = np.zeros(S, dtype=bool)                                   # may state s come from s - 2
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    v = np.full(S, -np.inf)
    v[0] = lp[0, blank]
    if S > 1:
        v[1] = lp[0, ext[1]]
    back = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        a1 = np.full(S, -np.inf)
        a1[1:] = v[:-1]
        a2 = np.full(S, -np.inf)
        a2[2:] = v[:-2]
        a2[~skip] = -np.inf
        best, b = v.copy(), np.zeros(S, dtype=np.int8)
        m = a1 > best                                                # strictly better only: an equal value stays with s
        best[m], b[m] = a1[m], 1
        m = a2 > best
        best[m], b[m] = a2[m], 2
        v = best + lp[t, ext]
        back[t] = b
    s, score = S - 1, v[S - 1]
    if S > 1 and v[S - 2] > score:                                   # an equal value stays with the final blank
        s, score = S - 2, v[S - 2]
    if score == -np.inf:
        return none
    states = np.zeros(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(back[t, s])
    start, end, logp = np.full(L, -1, np.int64), np.full(L, -1, np.int64), np.zeros(L)
    for i in range(L):
        frames = np.nonzero(states == 2 * i + 1)[0]
        start[i], end[i] = frames[0], frames[-1]
        logp[i] = lp[frames, target[i]].sum()
    return Aligned(score, states, start, end, logp)


def rescore(lp, frame_state, target, blank=0):
    """Sum of the log-probabilities along a given path of lattice states (float64)."""
    ext = extended(target, blank)
    st = np.asarray(frame_state, dtype=np.int64)
    return float(np.asarray(lp, dtype=np.float64)[np.arange(len(st)), ext[st]].sum())


def collapses_to(frame_state, target, blank=0):
    """Is the path a valid CTC alignment of the target: starts in state 0 or 1, ends in 2L or 2L - 1, moves by 0, 1 or (between
    different labels) 2 states per frame, and its labels collapse (repeats merged, blanks dropped) to the target."""
    target = [int(c) for c in np.asarray(target).reshape(-1)]
    ext = extended(target, blank)
    st = [int(s) for s in np.asarray(frame_state).reshape(-1)]
    S = len(ext)
    if not st or min(st) < 0 or max(st) >= S or st[0] > 1 or st[-1] < S - 2:
        return False
    for a, b in zip(st[:-1], st[1:]):
        if b - a not in (0, 1, 2) or (b - a == 2 and not (b & 1 and ext[b] != ext[a])):
            return False
    lab = [int(ext[s]) for s in st]
    out = [c for k, c in enumerate(lab) if c != blank and (k == 0 or lab[k - 1] != c)]
    return out == target
