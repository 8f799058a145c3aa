"""Hot phrases for the device beam search (ds2_beam_decode_hot and its siblings; DESIGN.md "ds2_beam", hot words).

Host side only, numpy only.  A hot phrase is a string of words over the labels, joined by single spaces, with a weight w >= 0 in
natural-log units per non-space label.  From a list of phrases one open-addressing table is built for the kernel, laid out like
the tables of lm.py (16-byte entries [key, value], linear probing, power-of-two size, load <= 1/2):

  key    the 61-bit polynomial hash of a phrase prefix's label string, the space label included (lm.hash_labels: the recurrence of
         the beam strings, started from HASH_EMPTY); one entry for every non-empty prefix q of every phrase
  value  bits 0 .. 31   v(q) = max over the phrases that start with q of fp32(w * n(q)), n(q) = the non-space labels of q
         bits 32 .. 62  c(q) = fp32(w * n(q)) of the phrase q itself (0 when q is no whole phrase); c >= 0, so its sign bit is free
         bit 63         q is a whole phrase

The products are formed in fp64 from the fp32 weight and rounded once; the device multiplies nothing.  The build raises when two
prefixes have the same hash or one has the hash of the empty string, so a lookup is exact.
"""
import math

import numpy as np

from . import lm as _lm

COMPLETE_BIT = 1 << 63


def normalize(hotwords, default_weight):
    """[(phrase, fp32 weight as a Python float), ...] from a list of strings or (string, weight) pairs."""
    out = []
    for item in hotwords or []:
        if isinstance(item, str):
            phrase, w = item, default_weight
        else:
            try:
                phrase, w = item
            except (TypeError, ValueError):
                raise ValueError("a hot word is a string or a (string, weight) pair, got %r" % (item,))
            if not isinstance(phrase, str):
                raise ValueError("a hot word is a string or a (string, weight) pair, got %r" % (item,))
        try:
            w = float(w)
        except (TypeError, ValueError):
            raise ValueError("hot phrase %r: the weight %r is no number" % (phrase, w))
        with np.errstate(over="ignore"):
            w32 = float(np.float32(w)) if math.isfinite(w) else w
        if not math.isfinite(w32) or w < 0:
            raise ValueError("hot phrase %r: the weight must be a finite fp32 value >= 0, got %r" % (phrase, w))
        out.append((phrase, w32))
    return out


def phrase_labels(phrase, labels, blank, space):
    """The label ids of a phrase; ValueError (naming the phrase) when it breaks a rule."""
    if not phrase:
        raise ValueError("hot phrase %r is empty" % phrase)
    sp = labels[space]
    if phrase[0] == sp or phrase[-1] == sp:
        raise ValueError("hot phrase %r starts or ends with a space" % phrase)
    if sp + sp in phrase:
        raise ValueError("hot phrase %r contains a double space" % phrase)
    index = {c: i for i, c in enumerate(labels) if i != blank}
    ids = []
    for ch in phrase:
        if ch not in index:
            raise ValueError("hot phrase %r contains %r, which is the blank or no label" % (phrase, ch))
        ids.append(index[ch])
    return tuple(ids)


def check_space(labels, blank):
    """The space label's index; ValueError when the labels have none besides the blank."""
    if ' ' not in labels or labels.index(' ') == blank:
        raise ValueError("hot words need a space label other than the blank to end words")
    return labels.index(' ')


def prefix_values(hotwords, labels, blank, default_weight=2.0):
    """{prefix label tuple: (v, complete, c)} over every non-empty prefix of every phrase (v, c: np.float32).  Every ValueError of
    the phrase rules is raised here."""
    space = check_space(labels, blank)
    items = normalize(hotwords, default_weight)
    seen, phrases = {}, []
    for phrase, w in items:
        ids = phrase_labels(phrase, labels, blank, space)
        if ids in seen:
            raise ValueError("hot phrase %r is listed twice" % phrase)
        seen[ids] = phrase
        phrases.append((phrase, ids, w))
    for phrase, ids, _ in phrases:
        for other, oids, _ in phrases:
            if len(oids) > len(ids) + 1 and oids[:len(ids)] == ids and oids[len(ids)] == space:
                raise ValueError("hot phrase %r followed by a space is a prefix of %r: nested phrases are not supported, list the "
                                 "remainder %r as a phrase of its own" % (phrase, other, other[len(phrase) + 1:]))
    out = {}
    for phrase, ids, w in phrases:
        n = 0
        for k, c in enumerate(ids):
            n += c != space
            with np.errstate(over="ignore"):
                val = np.float32(np.float64(w) * n)           # fp64 product of the fp32 weight, rounded once
            if not np.isfinite(val):
                raise ValueError("hot phrase %r: weight %r times %d labels is no finite fp32 value" % (phrase, w, n))
            q = ids[:k + 1]
            v, complete, cval = out.get(q, (np.float32(0), False, np.float32(0)))
            if k + 1 == len(ids):
                complete, cval = True, val
            out[q] = (max(v, val), complete, cval)
    return out


def build_table(hotwords, labels, blank, default_weight=2.0):
    """The hot-word table as an int64 array of shape (slots, 2).  ValueError for a phrase that breaks a rule and for two prefixes
    with one hash key."""
    pre = prefix_values(hotwords, labels, blank, default_weight)
    spelled = {_lm.HASH_EMPTY: ()}
    keys, vals = [], []
    for q, (v, complete, c) in pre.items():
        h = _lm.hash_labels(q)
        if spelled.setdefault(h, q) != q:
            raise ValueError("hot-word table: the prefixes %r and %r have the same hash key; lookups would not be exact"
                             % (''.join(labels[i] for i in spelled[h]), ''.join(labels[i] for i in q)))
        keys.append(h)
        vals.append(int(np.float32(v).view(np.uint32)) | (int(np.float32(c).view(np.uint32)) << 32) | (COMPLETE_BIT if complete else 0))
    return _lm.make_table(np.array(keys, np.uint64), np.array(vals, np.uint64), "hot-word table")


def lookup(table, key):
    """(v, complete, c) of a present key (v, c: np.float32), or None; the kernel's probe sequence."""
    val = _lm.table_find(table, key)
    if val is None:
        return None
    bits = np.array([val & 0xffffffff, (val >> 32) & 0x7fffffff], np.uint32).view(np.float32)
    return bits[0], bool(val >> 63), bits[1]
