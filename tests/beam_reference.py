"""Numpy restatement of the CTC prefix beam search that ds2_beam_decode implements (DESIGN.md "ds2_beam"; ctcdecode's
ctc_beam_search_decoder without a scorer).  It is written from the rules, not from the kernel: beams are label strings with
interned ids, extensions merge by string equality, nodes / offsets / tie-breaking follow the rules literally, and every step is
vectorised over (beam, kept class) with numpy so that the GPU tests can afford it.

dtype=np.float32 repeats the kernel's arithmetic operation for operation: fp32 additions, and every log / exp evaluated in fp64 and
rounded once to fp32 (the kernel does the same), so both give the same bits except in the rare double-rounding case and the
selection at every step -- exact ties included -- is the same.  dtype=np.float64 is the exact form the host tests compare with
brute force and torch's CTC loss.

Besides the beams it reports, per utterance, the smallest gap between the last kept and the first dropped candidate over all
steps (relative to the kept score), the smallest gap between adjacent output beams, and how often a pruned prefix was re-created
("revivals") and such a re-created prefix had an extension merge into a beam that hangs off its old node ("revival_merges")."""
import numpy as np

FLT_MIN = np.float32(np.finfo(np.float32).tiny)


def _lse(x, y, dt):
    # evaluated in fp64 and rounded once to dt, as the kernel does
    with np.errstate(invalid="ignore", over="ignore"):
        x64, y64 = x.astype(np.float64), y.astype(np.float64)
        m = np.maximum(x64, y64)
        r = (m + np.log(np.exp(x64 - m) + np.exp(y64 - m))).astype(dt)
    r = np.where(x == -np.inf, y, r)
    return np.where(y == -np.inf, x, r).astype(dt)


def prune(p, cutoff_top_n, cutoff_prob):
    """p: (T, C) float32 probabilities.  Returns per frame (kept classes, their probabilities as float32), kept classes in
    descending probability (lower class first on ties) when pruning applies, else all classes in index order."""
    T, C = p.shape
    cp = float(np.float32(cutoff_prob))                 # the ABI passes cutoff_prob as fp32
    K = min(int(cutoff_top_n), C)
    if not (cp < 1.0 or cutoff_top_n < C):
        return [(np.arange(C), p[t]) for t in range(T)]
    order = np.argsort(-p, axis=1, kind="stable")
    out = []
    for t in range(T):
        o = order[t]
        n = K
        if cp < 1.0:
            cum = np.cumsum(p[t, o].astype(np.float64))
            hit = np.nonzero(cum >= cp)[0]
            if len(hit):
                n = min(n, int(hit[0]) + 1)
        out.append((o[:n], p[t, o[:n]]))
    return out


def beam_search(p, size, blank, beam_width, cutoff_top_n=40, cutoff_prob=1.0, dtype=np.float32):
    """p: (T, C) probabilities of one utterance (float32); frames t < size are decoded.  Returns a dict:
    beams: list (rank order) of (labels tuple, frames tuple, score = -log p as float); boundary_gap, adjacent_gap (relative),
    revivals, revival_merges."""
    dt = np.dtype(dtype).type
    p = np.asarray(p, dtype=np.float32)
    size = max(0, min(int(size), p.shape[0]))
    B = int(beam_width)
    pruned = prune(p[:size], cutoff_top_n, cutoff_prob)
    # interned strings: sid -> (parent sid, label); sid 0 = the empty string
    intern, sid_parent = {}, [(-1, -1)]
    nodes = []                                          # node -> [parent node, label, frame]
    # beam arrays
    pb = np.array([0.0], dt)
    pnb = np.array([-np.inf], dt)
    lpc = np.array([-np.inf], dt)
    last = np.array([-1])
    sid = np.array([0])
    node = np.array([-1])
    ever = {0}
    boundary_gap, revivals, revival_merges = np.inf, 0, 0
    for t in range(size):
        kc, kp = pruned[t]
        klp = np.log(kp.astype(np.float64) + np.float64(FLT_MIN)).astype(dt)     # log(p + FLT_MIN) in fp64, kept as dt
        nb, nk = len(pb), len(kc)
        kpos = {int(c): k for k, c in enumerate(kc)}
        score = _lse(pb, pnb, dt)
        # extensions (i, k)
        same = kc[None, :] == last[:, None]
        M = (np.where(same, pb[:, None], score[:, None]) + klp[None, :]).astype(dt)
        M[:, kc == blank] = -np.inf
        # merges: beam j's parent string is a beam i and j's last label is kept -> (i, last_j) feeds j
        beam_of = {int(s): i for i, s in enumerate(sid)}
        ext_into = np.full(nb, -np.inf, dt)
        new_lpc = lpc.copy()
        for j in range(nb):
            if last[j] < 0 or int(last[j]) not in kpos:
                continue
            i = beam_of.get(sid_parent[sid[j]][0])
            if i is None:
                continue
            k = kpos[int(last[j])]
            ext_into[j] = M[i, k]
            M[i, k] = -np.inf                           # not a new candidate
            if klp[k] > lpc[j]:                         # the log_prob_c rule: a strictly larger lp moves the frame
                new_lpc[j] = klp[k]
                nodes[node[j]][2] = t
            if nodes[node[j]][0] != node[i]:
                revival_merges += 1
        # every beam itself
        kb = kpos.get(blank)
        npb = (score + klp[kb]).astype(dt) if kb is not None else np.full(nb, -np.inf, dt)
        lk = np.array([kpos.get(int(c), -1) for c in last])
        npnb = np.where(lk >= 0, pnb + klp[np.maximum(lk, 0)], -np.inf).astype(dt)
        npnb = _lse(npnb, ext_into, dt)
        stay = _lse(npb, npnb, dt)
        # candidates: beam itself (class key 0) and extension (class key c + 1); best score, then lower source rank, lower class
        cs = np.concatenate([stay, M.reshape(-1)])
        src = np.concatenate([np.arange(nb), np.repeat(np.arange(nb), nk)])
        cls1 = np.concatenate([np.zeros(nb, np.int64), np.tile(kc + 1, nb)])
        kind = np.concatenate([np.full(nb, -1), np.tile(np.arange(nk), nb)])
        fin = np.nonzero(cs > -np.inf)[0]
        order = fin[np.lexsort((cls1[fin], src[fin], -cs[fin].astype(np.float64)))]
        if len(order) > B:
            a, b = float(cs[order[B - 1]]), float(cs[order[B]])
            boundary_gap = min(boundary_gap, (a - b) / max(1.0, abs(a)))
        order = order[:B]
        n_pb, n_pnb, n_lpc, n_last, n_sid, n_node = [], [], [], [], [], []
        for r, q in enumerate(order):
            i, k = src[q], kind[q]
            if k < 0:
                n_pb.append(npb[i]); n_pnb.append(npnb[i]); n_lpc.append(new_lpc[i])
                n_last.append(last[i]); n_sid.append(sid[i]); n_node.append(node[i])
            else:
                c = int(kc[k])
                key = (int(sid[i]), c)
                s = intern.get(key)
                if s is None:
                    s = intern[key] = len(sid_parent)
                    sid_parent.append(key)
                if s in ever:
                    revivals += 1
                ever.add(s)
                nodes.append([int(node[i]), c, t])
                n_pb.append(dt(-np.inf)); n_pnb.append(cs[q]); n_lpc.append(klp[k])
                n_last.append(c); n_sid.append(s); n_node.append(len(nodes) - 1)
        pb, pnb, lpc = np.array(n_pb, dt), np.array(n_pnb, dt), np.array(n_lpc, dt)
        last, sid, node = np.array(n_last), np.array(n_sid), np.array(n_node)
    final = -_lse(pb, pnb, dt).astype(np.float64)
    beams = []
    for r in range(len(pb)):
        labels, frames, nd = [], [], int(node[r])
        while nd >= 0:
            labels.append(nodes[nd][1])
            frames.append(nodes[nd][2])
            nd = nodes[nd][0]
        beams.append((tuple(labels[::-1]), tuple(frames[::-1]), float(final[r]) + 0.0))
    adj = np.inf
    for r in range(1, len(final)):
        adj = min(adj, (final[r] - final[r - 1]) / max(1.0, abs(final[r])))
    return dict(beams=beams, boundary_gap=boundary_gap, adjacent_gap=adj, revivals=revivals, revival_merges=revival_merges)


def brute_force(p, size=None):
    """Exact -log p of every label string: all C^T paths, collapsed (repeats merged, blanks removed), summed in float64 over
    log(p + FLT_MIN).  Blank = 0.  Returns {labels tuple: -log p}."""
    import itertools
    p = np.asarray(p, dtype=np.float32)
    T = p.shape[0] if size is None else int(size)
    lp = np.log(p[:T].astype(np.float64) + np.float64(FLT_MIN))
    acc = {}
    for path in itertools.product(range(p.shape[1]), repeat=T):
        s = float(sum(lp[t, c] for t, c in enumerate(path)))
        lab, prev = [], -1
        for c in path:
            if c != 0 and c != prev:
                lab.append(c)
            prev = c
        key = tuple(lab)
        acc[key] = np.logaddexp(acc[key], s) if key in acc else s
    return {k: -v for k, v in acc.items()}
