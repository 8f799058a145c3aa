"""Numpy restatement of the CTC prefix beam search with hot words (ds2_beam_decode_hot, ds2_beam_decode_lm_hot), written from
the rules of DESIGN.md "ds2_beam" (hot words), not from the kernel.  It extends tests/beam_reference.py and
tests/beam_lm_reference.py: beams are label strings with interned ids, and what the hot words (and the language model, when there
is one) know of a string is derived from the string when it is first seen, by walking the rules over its labels.  The phrase table
is a dict keyed by label tuples; the hash table of the kernel plays no part here.

dtype=np.float32 repeats the kernel's arithmetic (fp32 sums in the stated association order; every log / exp and every word bonus
evaluated in fp64 and rounded once), dtype=np.float64 is the exact form that the host tests compare with brute force.  In both
the table's values are the fp32 products fp32(w * n), as the host builds them.

Besides the beams the search returns counters over the strings that were kept at some step (and, for the end of the utterance,
over the beams that are left): completions, breaks, fallbacks, covered out-of-vocabulary word events and lexicon rescues."""
import numpy as np

from beam_lm_reference import OOV
from beam_reference import FLT_MIN, _lse, prune

HOT = -2        # a covered out-of-vocabulary word in an LM context: matches no stored n-gram and is not the OOV mark


class HotTable:
    """phrases: [(label tuple, weight)].  entries[q] = (v, complete, c) for every non-empty prefix q of every phrase."""

    def __init__(self, phrases, space):
        self.space, self.entries = space, {}
        for ids, w in phrases:
            ids, w32 = tuple(int(c) for c in ids), np.float32(w)
            n = 0
            for k, c in enumerate(ids):
                n += c != space
                val = np.float32(np.float64(w32) * n)
                v, complete, cv = self.entries.get(ids[:k + 1], (np.float32(0), False, np.float32(0)))
                if k + 1 == len(ids):
                    complete, cv = True, val
                self.entries[ids[:k + 1]] = (max(v, val), complete, cv)

    def v(self, mu):
        return self.entries[mu][0] if mu else np.float32(0)

    def complete(self, mu):
        return bool(mu) and self.entries[mu][1]

    def c(self, mu):
        return self.entries[mu][2]

    def covered(self, mu):
        """whether a space after a string with match mu is covered"""
        return self.complete(mu) or (bool(mu) and mu + (self.space,) in self.entries)

    def extend(self, mu, part, done, c, dt):
        """(mu, done, what happened) of a string extended by label c, from its match, partial word and done; what happened is
        one of None, "completion", "break", "fallback" """
        if c != self.space:
            if mu and mu + (c,) in self.entries:
                return mu + (c,), done, None
            if part + (c,) in self.entries:
                return part + (c,), done, "fallback" if mu else None
            return (), done, "break" if mu else None
        if self.complete(mu):
            return (), dt(done + dt(self.c(mu))), "completion"
        if mu and mu + (c,) in self.entries:
            return mu + (c,), done, None
        return (), done, "break" if mu else None

    def hot(self, mu, done, dt):
        return dt(done + dt(self.v(mu)))

    def hot_end(self, mu, done, dt):
        return dt(done + dt(self.c(mu))) if self.complete(mu) else done


def walk(table, labels, dtype=np.float32):
    """(mu, done, events) of a label string by the rules, label by label"""
    dt = np.dtype(dtype).type
    mu, part, done, events = (), (), dt(0.0), []
    for c in labels:
        mu, done, what = table.extend(mu, part, done, int(c), dt)
        part = () if c == table.space else part + (int(c),)
        events.append(what)
    return mu, done, events


def beam_search_hot(p, size, blank, beam_width, cutoff_top_n, cutoff_prob, table, scorer=None, hot_oov_logp=-11.5,
                    dtype=np.float32):
    """p: (T, C) probabilities of one utterance; frames t < size are decoded.  table: a HotTable; scorer: None or the Scorer of
    beam_lm_reference (its dtype is the search's).  Returns a dict: beams = list (rank order) of (labels tuple, frames tuple,
    total score = -(log p + lm + hot_end), acoustic score = -log p); adjacent_gap (relative, of the totals); the counters."""
    sc = scorer
    dt = sc.dt if sc is not None else np.dtype(dtype).type
    space = table.space
    p = np.asarray(p, dtype=np.float32)
    size = max(0, min(int(size), p.shape[0]))
    B = int(beam_width)
    pruned = prune(p[:size], cutoff_top_n, cutoff_prob)
    intern, sid_parent = {}, [(-1, -1)]
    # what is known of string sid: (partial word, match, done, LM context, lm)
    info = [((), (), dt(0.0), sc.start if sc is not None else (), dt(0.0))]
    nodes = []
    pb, pnb, lpc = np.array([0.0], dt), np.array([-np.inf], dt), np.array([-np.inf], dt)
    last, sid, node = np.array([-1]), np.array([0]), np.array([-1])
    count = dict(completions=0, breaks=0, fallbacks=0, covered_oov=0, lexicon_rescues=0, word_events=0)
    # the ABI passes hot_oov_logp as fp32; the bonus is formed in fp64 and rounded once
    oov_bonus = None if sc is None else dt(sc.alpha * float(np.float32(hot_oov_logp)) + sc.beta)

    def word_event(part, mu, ctx, end):
        """(bonus, id that enters the context, covered out-of-vocabulary) of the word event of partial word `part`"""
        wid = sc.words.get(part, OOV)
        if wid == OOV and (table.complete(mu) if end else table.covered(mu)):
            return oov_bonus, HOT, True
        return sc.bonus(wid, ctx), wid, False

    def extension(s, c):
        """(lm, hot, rescued) of string s extended by c; lm None: the extension does not exist"""
        part, mu, done, ctx, lm = info[s]
        mu2, done2, _ = table.extend(mu, part, done, c, dt)
        hot = table.hot(mu2, done2, dt)
        if sc is None:
            return dt(0.0), hot, False
        if c != space:
            if sc.lexicon and part + (c,) not in sc.prefixes:
                return (lm, hot, True) if mu2 else (None, hot, False)
            return lm, hot, False
        if not part:
            return (None if sc.lexicon else lm), hot, False          # space after space (or at the start): no word event
        known = part in sc.words
        if sc.lexicon and not known and not table.covered(mu):
            return None, hot, False
        return dt(lm + word_event(part, mu, ctx, False)[0]), hot, sc.lexicon and not known

    rows = {}

    def ext_rows(s):
        if s not in rows:
            L, H = np.full(p.shape[1], -np.inf, dt), np.zeros(p.shape[1], dt)
            for c in range(p.shape[1]):
                if c != blank:
                    l, H[c], _ = extension(s, c)
                    L[c] = -np.inf if l is None else l
            rows[s] = (L, H)
        return rows[s]

    for t in range(size):
        if len(pb) == 0:
            break
        kc, kp = pruned[t]
        klp = np.log(kp.astype(np.float64) + np.float64(FLT_MIN)).astype(dt)
        nb, nk = len(pb), len(kc)
        kpos = {int(c): k for k, c in enumerate(kc)}
        score = _lse(pb, pnb, dt)
        lm_b = np.array([info[s][4] for s in sid], dt)
        hot_b = np.array([table.hot(info[s][1], info[s][2], dt) for s in sid], dt)
        same = kc[None, :] == last[:, None]
        M = (np.where(same, pb[:, None], score[:, None]) + klp[None, :]).astype(dt)      # acoustic mass of extension (i, k)
        M[:, kc == blank] = -np.inf
        L = np.stack([ext_rows(s)[0] for s in sid])[:, kc].astype(dt)
        H = np.stack([ext_rows(s)[1] for s in sid])[:, kc].astype(dt)
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
            ext_into[j] = M[i, k]
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
            if sc is None:                                  # lse + hot; with an LM (lse + lm) + hot
                stay = (_lse(npb, npnb, dt) + hot_b).astype(dt)
                ext = (M + H).astype(dt)
            else:
                stay = ((_lse(npb, npnb, dt) + lm_b).astype(dt) + hot_b).astype(dt)
                ext = ((M + L).astype(dt) + H).astype(dt)
            ext = np.where(merged, -np.inf, ext).astype(dt)
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
                part, mu, done, ctx, lm = info[sid[i]]
                mu2, done2, what = table.extend(mu, part, done, c, dt)
                count["completions"] += what == "completion"
                count["breaks"] += what == "break"
                count["fallbacks"] += what == "fallback"
                l, _, rescued = extension(int(sid[i]), c)
                count["lexicon_rescues"] += bool(rescued)
                if c == space:
                    if sc is not None and part:
                        _, wid, cov = word_event(part, mu, ctx, False)
                        count["word_events"] += 1
                        count["covered_oov"] += cov
                        ctx = sc.shift(ctx, wid)
                    info.append(((), mu2, done2, ctx, l))
                else:
                    info.append((part + (c,), mu2, done2, ctx, l))
            nodes.append([int(node[i]), c, t])
            n_pb.append(dt(-np.inf)); n_pnb.append(M[i, k]); n_lpc.append(klp[k])
            n_last.append(c); n_sid.append(s); n_node.append(len(nodes) - 1)
        pb, pnb, lpc = np.array(n_pb, dt), np.array(n_pnb, dt), np.array(n_lpc, dt)
        last, sid, node = np.array(n_last), np.array(n_sid), np.array(n_node)
    # end of utterance: the LM's bonus for a beam that ends inside a word, and hot_end
    ac = _lse(pb, pnb, dt)
    total = np.zeros(len(pb), dt)
    for r in range(len(pb)):
        part, mu, done, ctx, lm = info[sid[r]]
        if sc is not None and part:
            bonus, _, cov = word_event(part, mu, ctx, True)
            lm = dt(lm + bonus)
            count["word_events"] += 1
            count["covered_oov"] += cov
        count["completions"] += table.complete(mu)
        he = table.hot_end(mu, done, dt)
        total[r] = dt(dt(ac[r] + lm) + he) if sc is not None else dt(ac[r] + he)
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
    return dict(beams=beams, adjacent_gap=adj, **count)
