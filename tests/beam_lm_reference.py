"""Numpy restatement of the CTC prefix beam search with a word n-gram language model (ds2_beam_decode_lm), written from the
rules of DESIGN.md "ds2_beam" (language model), not from the kernel.  It extends tests/beam_reference.py: beams are label strings
with interned ids, and what the language model knows of a string (its partial word, its context of completed words, the fp32 sum
of its word bonuses) is derived from the string when the string is first seen, by walking the rules over its labels.  The model
is the parsed ARPA file (lm.ArpaLM.ngrams: dicts keyed by id tuples); the hash tables of the kernel play no part here.

dtype=np.float32 repeats the kernel's arithmetic (fp32 sums; every log / exp and every word bonus evaluated in fp64 and rounded
once), dtype=np.float64 is the exact form that the host tests compare with brute force."""
import numpy as np

from beam_reference import FLT_MIN, _lse, prune

LOG10_E = 0.4342944819032518
OOV_SCORE = -1000.0
OOV = -1


class Scorer:
    """The scoring rules over word ids.  A context is a tuple of the ids of the last order - 1 completed words, oldest first
    (<s> while fewer exist, OOV for a word outside the vocabulary)."""

    def __init__(self, lm, labels, blank, alpha, beta, lexicon=True, dtype=np.float32):
        self.lm, self.order, self.lexicon = lm, lm.order, bool(lexicon)
        self.dt = np.dtype(dtype).type
        self.alpha, self.beta = float(np.float32(alpha)), float(np.float32(beta))    # the ABI passes both as fp32
        self.blank, self.space = blank, labels.index(' ')
        spell = {c: i for i, c in enumerate(labels) if i not in (blank, self.space)}
        self.words, self.prefixes = {}, set()
        for wid, w in enumerate(lm.words):
            if w and all(ch in spell for ch in w):
                lab = tuple(spell[ch] for ch in w)
                self.words[lab] = wid
                for n in range(1, len(lab) + 1):
                    self.prefixes.add(lab[:n])
        self.start = (lm.word_id["<s>"],) * (self.order - 1)
        self._memo = {}

    def ln_p(self, wid, ctx):
        """ln P(word | context): the longest stored n-gram ending in the word; every shorter step first adds the backoff of the
        context it drops (0 when that context is not stored).  log10 terms (fp32) summed in fp64 in that order, then / log10(e)."""
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


def beam_search_lm(p, size, blank, beam_width, cutoff_top_n, cutoff_prob, scorer):
    """p: (T, C) probabilities of one utterance; frames t < size are decoded.  Returns a dict: beams = list (rank order) of
    (labels tuple, frames tuple, total score = -(log p + lm), acoustic score = -log p); adjacent_gap (relative, of the totals);
    word_events / oov_events: word bonuses (and those with ln P = -1000) charged to beams that were kept at some step or at the end."""
    dt, sc = scorer.dt, scorer
    p = np.asarray(p, dtype=np.float32)
    size = max(0, min(int(size), p.shape[0]))
    B = int(beam_width)
    pruned = prune(p[:size], cutoff_top_n, cutoff_prob)
    intern, sid_parent = {}, [(-1, -1)]
    # what the language model knows of string sid: (partial word as labels, context, lm)
    info = [((), sc.start, dt(0.0))]
    nodes = []
    pb, pnb, lpc = np.array([0.0], dt), np.array([-np.inf], dt), np.array([-np.inf], dt)
    last, sid, node = np.array([-1]), np.array([0]), np.array([-1])
    word_events = oov_events = 0

    def space_lm(s):
        """lm of string s extended by the space label (None: the extension does not exist) and whether it is a word event"""
        part, ctx, lm = info[s]
        if not part:
            return (None if sc.lexicon else lm), False           # space after space (or at the start): no word event
        wid = sc.words.get(part, OOV)
        if sc.lexicon and wid == OOV:
            return None, False
        return dt(lm + sc.bonus(wid, ctx)), True

    rows = {}

    def ext_lm(s):
        """per class c: the lm of string s extended by c, -inf where the lexicon drops the extension"""
        if s not in rows:
            part, _, lm = info[s]
            row = np.full(p.shape[1], lm, dt)
            if sc.lexicon:
                for c in range(p.shape[1]):
                    if c != blank and c != sc.space and part + (c,) not in sc.prefixes:
                        row[c] = -np.inf
            l, _ = space_lm(s)
            row[sc.space] = -np.inf if l is None else l
            rows[s] = row
        return rows[s]

    for t in range(size):
        if len(pb) == 0:                  # lexicon mode with pruning can leave a frame without any candidate: no beam survives
            break
        kc, kp = pruned[t]
        klp = np.log(kp.astype(np.float64) + np.float64(FLT_MIN)).astype(dt)
        nb, nk = len(pb), len(kc)
        kpos = {int(c): k for k, c in enumerate(kc)}
        score = _lse(pb, pnb, dt)
        lm_b = np.array([info[s][2] for s in sid], dt)
        same = kc[None, :] == last[:, None]
        M = (np.where(same, pb[:, None], score[:, None]) + klp[None, :]).astype(dt)      # acoustic mass of extension (i, k)
        M[:, kc == blank] = -np.inf
        # the language model's part of extension (i, k): lm_i, with the word bonus at the space label; -inf where the lexicon drops it
        L = np.stack([ext_lm(s) for s in sid])[:, kc].astype(dt)
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
                part, ctx, lm = info[sid[i]]
                if c == sc.space:
                    l, event = space_lm(sid[i])
                    if event:
                        wid = sc.words.get(part, OOV)
                        word_events += 1
                        oov_events += wid == OOV or OOV in ctx
                        ctx = sc.shift(ctx, wid)
                    info.append(((), ctx, l))
                else:
                    info.append((part + (c,), ctx, lm))
            nodes.append([int(node[i]), c, t])
            n_pb.append(dt(-np.inf)); n_pnb.append(M[i, k]); n_lpc.append(klp[k])
            n_last.append(c); n_sid.append(s); n_node.append(len(nodes) - 1)
        pb, pnb, lpc = np.array(n_pb, dt), np.array(n_pnb, dt), np.array(n_lpc, dt)
        last, sid, node = np.array(n_last), np.array(n_sid), np.array(n_node)
    # end of utterance: a beam that ends inside a word gets that word's bonus (a mere prefix counts as OOV in lexicon mode)
    ac = _lse(pb, pnb, dt)
    total = np.zeros(len(pb), dt)
    for r in range(len(pb)):
        part, ctx, lm = info[sid[r]]
        if part:
            wid = sc.words.get(part, OOV)
            lm = dt(lm + sc.bonus(wid, ctx))
            word_events += 1
            oov_events += wid == OOV or OOV in ctx
        total[r] = dt(ac[r] + lm)
    rank = np.lexsort((np.arange(len(pb)), -total.astype(np.float64)))          # by total, ties to the earlier rank
    beams = []
    for r in rank:
        labels, frames, nd = [], [], int(node[r])
        while nd >= 0:
            labels.append(nodes[nd][1])
            frames.append(nodes[nd][2])
            nd = nodes[nd][0]
        beams.append((tuple(labels[::-1]), tuple(frames[::-1]), -float(total[r]) + 0.0, -float(ac[r]) + 0.0))
    adj = np.inf
    for r in range(1, len(beams)):
        adj = min(adj, (beams[r][2] - beams[r - 1][2]) / max(1.0, abs(beams[r][2])))
    return dict(beams=beams, adjacent_gap=adj, word_events=word_events, oov_events=oov_events)
