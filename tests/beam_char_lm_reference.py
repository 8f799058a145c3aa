"""Numpy restatement of the CTC prefix beam search with a character n-gram language model (ds2_beam_decode_clm), written from the
rules of DESIGN.md "ds2_beam" (character language model), not from the kernel.  It extends tests/beam_reference.py the way
tests/beam_lm_reference.py does: beams are label strings with interned ids, and what the model knows of a string (the ids of its
last order - 1 labels and the fp32 sum of its label bonuses) is derived from the string when the string is first seen.  The
model is the parsed ARPA file (lm.ArpaLM.ngrams: dicts keyed by id tuples); the kernel's hash tables play no part here, and the
label ids are looked up here, not taken from lm.char_ids.

dtype=np.float32 repeats the kernel's arithmetic (fp32 sums; every log / exp and every bonus evaluated in fp64 and rounded once),
dtype=np.float64 is the exact form that the host tests compare with brute force."""
import numpy as np

from beam_reference import FLT_MIN, _lse, prune

LOG10_E = 0.4342944819032518
OOV_SCORE = -1000.0
OOV = -1


class CharScorer:
    """The scoring rules over label ids.  A context is a tuple of the unigram ids of the last order - 1 labels, oldest first (<s>
    while fewer exist, OOV for a label whose token is no unigram)."""

    def __init__(self, lm, labels, blank, alpha, beta, space_token=None, dtype=np.float32):
        self.lm, self.order = lm, lm.order
        self.dt = np.dtype(dtype).type
        self.alpha, self.beta = float(np.float32(alpha)), float(np.float32(beta))    # the ABI passes both as fp32
        self.blank = blank
        if space_token is not None and space_token not in lm.word_id:
            raise ValueError("space_token %r is no unigram" % (space_token,))
        self.cid = []
        for c, tok in enumerate(labels):
            if tok == " " and space_token is not None:
                tok = space_token
            self.cid.append(OOV if c == blank else lm.word_id.get(tok, OOV))
        self.start = (lm.word_id["<s>"],) * (self.order - 1)
        self._memo = {}

    def ln_p(self, wid, ctx):
        """ln P(label | context): the longest stored n-gram ending in the label; every shorter step first adds the backoff of the
        context it drops (0 when that context is not stored).  log10 terms (fp32) summed in fp64 in that order, then / log10(e).
        -1000 when the label or any context id is OOV, or when nothing is stored."""
        if wid == OOV or OOV in ctx:
            return OOV_SCORE
        acc, ctx = 0.0, tuple(ctx)
        while True:
            hit = self.lm.ngrams[len(ctx)].get(ctx + (wid,))
            if hit is not None:
                return (acc + float(hit[0])) / LOG10_E
            if not ctx:
                return OOV_SCORE
            back = self.lm.ngrams[len(ctx) - 1].get(ctx)
            acc += float(back[1]) if back is not None else 0.0
            ctx = ctx[1:]

    def bonus(self, wid, ctx):
        key = (wid, ctx)
        if key not in self._memo:
            self._memo[key] = self.dt(self.alpha * self.ln_p(wid, ctx) + self.beta)     # formed in fp64, rounded once
        return self._memo[key]

    def shift(self, ctx, wid):
        return (ctx + (wid,))[1:] if self.order > 1 else ()

    def string_lm(self, labels):
        """(lm, context) of a label string by the rules alone: the sum of its label bonuses, in order, in the scorer's dtype"""
        lm, ctx = self.dt(0.0), self.start
        for c in labels:
            lm = self.dt(lm + self.bonus(self.cid[c], ctx))
            ctx = self.shift(ctx, self.cid[c])
        return lm, ctx


def beam_search_clm(p, size, blank, beam_width, cutoff_top_n, cutoff_prob, scorer):
    """p: (T, C) probabilities of one utterance; frames t < size are decoded.  Returns a dict: beams = list (rank order: the last
    selection's) of (labels tuple, frames tuple, total score = -(log p + lm), acoustic score = -log p); adjacent_gap (relative, of
    the totals); label_events / oov_events: bonuses (and those with ln P = -1000) of the strings that were created."""
    dt, sc = scorer.dt, scorer
    p = np.asarray(p, dtype=np.float32)
    size = max(0, min(int(size), p.shape[0]))
    B = int(beam_width)
    pruned = prune(p[:size], cutoff_top_n, cutoff_prob)
    intern, sid_parent = {}, [(-1, -1)]
    info = [(sc.start, dt(0.0))]                        # string sid -> (context, lm)
    nodes = []
    pb, pnb, lpc = np.array([0.0], dt), np.array([-np.inf], dt), np.array([-np.inf], dt)
    last, sid, node = np.array([-1]), np.array([0]), np.array([-1])
    label_events = oov_events = 0
    rows = {}
    for t in range(size):
        kc, kp = pruned[t]
        klp = np.log(kp.astype(np.float64) + np.float64(FLT_MIN)).astype(dt)
        nb, nk = len(pb), len(kc)
        kpos = {int(c): k for k, c in enumerate(kc)}
        score = _lse(pb, pnb, dt)
        lm_b = np.array([info[s][1] for s in sid], dt)
        same = kc[None, :] == last[:, None]
        M = (np.where(same, pb[:, None], score[:, None]) + klp[None, :]).astype(dt)      # acoustic mass of extension (i, k)
        M[:, kc == blank] = -np.inf
        # the lm of the string that extension (i, k) creates: lm_i + bonus(label | context of i)
        # (kept per string and class once formed: a string's row does not change while it stays a beam)
        L = np.zeros((nb, nk), dt)
        for i, s in enumerate(sid):
            ctx, lm = info[s]
            row = rows.setdefault(int(s), np.full(p.shape[1], np.nan, dt))
            for c in kc[np.isnan(row[kc])]:
                row[c] = dt(lm + sc.bonus(sc.cid[int(c)], ctx)) if c != blank else 0.0
            L[i] = row[kc]
        beam_of = {int(s): i for i, s in enumerate(sid)}
        ext_into = np.full(nb, -np.inf, dt)
        new_lpc = lpc.copy()
        merged = np.zeros((nb, nk), bool)
        for j in range(nb):
            if last[j] < 0 or int(last[j]) not in kpos:
                continue
            i = beam_of.get(sid_parent[sid[j]][0])
            if i is None:
                continue
            k = kpos[int(last[j])]
            ext_into[j] = M[i, k]                       # all paths into one string carry the same lm: only the mass moves
            merged[i, k] = True
            if klp[k] > lpc[j]:
                new_lpc[j] = klp[k]
                nodes[node[j]][2] = t
        kb = kpos.get(blank)
        npb = (score + klp[kb]).astype(dt) if kb is not None else np.full(nb, -np.inf, dt)
        lk = np.array([kpos.get(int(c), -1) for c in last])
        npnb = np.where(lk >= 0, pnb + klp[np.maximum(lk, 0)], -np.inf).astype(dt)
        npnb = _lse(npnb, ext_into, dt)
        with np.errstate(invalid="ignore"):
            stay = (_lse(npb, npnb, dt) + lm_b).astype(dt)
            ext = np.where(merged, -np.inf, (M + L).astype(dt)).astype(dt)
        cs = np.concatenate([stay, ext.reshape(-1)])
        src = np.concatenate([np.arange(nb), np.repeat(np.arange(nb), nk)])
        cls1 = np.concatenate([np.zeros(nb, np.int64), np.tile(kc + 1, nb)])
        kind = np.concatenate([np.full(nb, -1), np.tile(np.arange(nk), nb)])
        fin = np.nonzero(cs > -np.inf)[0]
        order = fin[np.lexsort((cls1[fin], src[fin], -cs[fin].astype(np.float64)))][:B]
        n_pb, n_pnb, n_lpc, n_last, n_sid, n_node = [], [], [], [], [], []
        for q in order:
            i, k = src[q], kind[q]
            if k < 0:
                n_pb.append(npb[i]); n_pnb.append(npnb[i]); n_lpc.append(new_lpc[i])
                n_last.append(last[i]); n_sid.append(sid[i]); n_node.append(node[i])
                continue
            c = int(kc[k])
            key = (int(sid[i]), c)
            s = intern.get(key)
            if s is None:
                s = intern[key] = len(sid_parent)
                sid_parent.append(key)
                ctx, lm = info[sid[i]]
                wid = sc.cid[c]
                label_events += 1
                oov_events += wid == OOV or OOV in ctx
                info.append((sc.shift(ctx, wid), L[i, k]))
            nodes.append([int(node[i]), c, t])
            n_pb.append(dt(-np.inf)); n_pnb.append(M[i, k]); n_lpc.append(klp[k])
            n_last.append(c); n_sid.append(s); n_node.append(len(nodes) - 1)
        pb, pnb, lpc = np.array(n_pb, dt), np.array(n_pnb, dt), np.array(n_lpc, dt)
        last, sid, node = np.array(n_last), np.array(n_sid), np.array(n_node)
    # no end-of-utterance term and no re-rank: the ranks are the last selection's
    ac = _lse(pb, pnb, dt)
    beams = []
    for r in range(len(pb)):
        total = dt(ac[r] + info[sid[r]][1])
        labels, frames, nd = [], [], int(node[r])
        while nd >= 0:
            labels.append(nodes[nd][1])
            frames.append(nodes[nd][2])
            nd = nodes[nd][0]
        beams.append((tuple(labels[::-1]), tuple(frames[::-1]), -float(total) + 0.0, -float(ac[r]) + 0.0))
    adj = np.inf
    for r in range(1, len(beams)):
        adj = min(adj, (beams[r][2] - beams[r - 1][2]) / max(1.0, abs(beams[r][2])))
    return dict(beams=beams, adjacent_gap=adj, label_events=label_events, oov_events=oov_events)
