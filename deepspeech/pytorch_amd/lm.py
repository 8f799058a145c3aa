"""Word n-gram language models for the device beam search (ds2_beam_decode_lm; DESIGN.md "ds2_beam", language model).

Host side only, numpy only: an ARPA text file (order 1 to 5) is parsed into per-order arrays, and from those two
open-addressing tables (load <= 1/2, linear probing, power-of-two sizes) are built for the kernel:

  word table    key = 61-bit polynomial hash of a word prefix's label string (the recurrence of the beam strings, hash_ext in
                ds2_beam.hip, started from HASH_EMPTY); one entry for every non-empty prefix of every vocabulary word that can be
                spelled with the labels; value = word id, or -1 for a proper prefix that is no word itself
  n-gram table  key = 64-bit hash of the id tuple, read from the last id to the first (so the keys of all suffixes of
                (context, word) come out of one pass); value = (log10 p, log10 backoff) as two fp32 bit patterns in one word

Both are int64 arrays of shape (slots, 2): [key, value]; a free slot holds EMPTY_KEY.  The build raises when two inserted keys
are equal, so the lookup of a present key is exact.  KenLM's binary format is not read (it needs KenLM itself).

A character model (ds2_beam_decode_clm; DESIGN.md "ds2_beam", character language model) is the same file read with the labels
as its units: char_ids maps every label to its unigram id, the n-gram table is the same, and there is no word table.
"""
import numpy as np

MASK64 = (1 << 64) - 1
M61 = (1 << 61) - 1
HASH_BASE = 0x0b7e151628aed2a7
HASH_EMPTY = 0x1f3d5b79a2c4e6f8 % M61
NGRAM_SEED = 0x243f6a8885a308d3
NGRAM_MUL = 0x9e3779b97f4a7c15
EMPTY_KEY = MASK64                      # never a 61-bit string hash; the build refuses an n-gram key equal to it
MAX_ORDER = 5
LOG10_E = 0.4342944819032518            # the divisor of ln P = log10 P / log10(e); the kernel uses the same literal
OOV_SCORE = -1000.0                     # ln P of a word event with an out-of-vocabulary word or context (ctcdecode's OOV_SCORE)
WORD_ABSENT, WORD_PREFIX = -2, -1       # word-table answers besides a word id


def hash_ext(h, c):
    """hash(s + c) of the beam strings: (hash(s) * base + c + 1) mod (2^61 - 1)."""
    return (h * HASH_BASE + c + 1) % M61


def hash_labels(label_ids):
    h = HASH_EMPTY
    for c in label_ids:
        h = hash_ext(h, int(c))
    return h


def ngram_mix(h, wid):
    t = ((h ^ (int(wid) + 1)) * NGRAM_MUL) & MASK64
    return t ^ (t >> 29)


def ngram_key(ids):
    """64-bit key of an id tuple (oldest word first), hashed from the last id to the first."""
    h = NGRAM_SEED
    for wid in reversed(ids):
        h = ngram_mix(h, wid)
    return h


def slot_of(key, mask):
    return (key ^ (key >> 32)) & mask


class ArpaLM:
    """A parsed ARPA file.  words[i] is the word of id i (ids in the order of the unigram section; <s>, </s>, <unk> are ordinary
    entries).  ids[m] is an (count, m + 1) int32 array of the (m + 1)-grams, logp[m] / backoff[m] their fp32 log10 values (backoff
    0 where the file gives none)."""

    def __init__(self, words, ids, logp, backoff, counts):
        self.words, self.ids, self.logp, self.backoff, self.counts = words, ids, logp, backoff, counts
        self.order = len(ids)
        self.word_id = {w: i for i, w in enumerate(words)}
        self._dicts = None

    @property
    def ngrams(self):
        """Per order a dict {id tuple: (log10 p, log10 backoff)} (fp32 values), for host-side scoring."""
        if self._dicts is None:
            self._dicts = [{tuple(int(v) for v in row): (p, b) for row, p, b in zip(self.ids[m], self.logp[m], self.backoff[m])}
                           for m in range(self.order)]
        return self._dicts

    @property
    def bos(self):
        return self.word_id["<s>"]


def load_arpa(path):
    """Parses an ARPA text file of order 1 to 5.  ValueError for anything else (a KenLM binary, a truncated or malformed file)."""
    def bad(why):
        return ValueError("%s is not a usable ARPA language model: %s (only ARPA text files load; other formats such as KenLM "
                          "binaries are not implemented)" % (path, why))
    try:
        with open(path, "rb") as f:
            raw = f.read()
    except OSError as e:
        raise bad("it cannot be read (%s)" % e.strerror)
    if raw.lstrip()[:6] != b"\\data\\":
        raise bad("it does not start with a \\data\\ section")
    try:
        lines = raw.decode("utf-8").split("\n")
    except UnicodeDecodeError:
        raise bad("it is not UTF-8 text")
    pos = 0
    while lines[pos].strip() != "\\data\\":
        pos += 1
    pos += 1
    counts = []
    while pos < len(lines) and not lines[pos].startswith("\\"):
        ln = lines[pos].strip()
        pos += 1
        if not ln:
            continue
        if not ln.startswith("ngram ") or "=" not in ln:
            raise bad("unexpected line %r in the \\data\\ section" % ln)
        m, cnt = ln[6:].split("=")
        try:
            m, cnt = int(m), int(cnt)
        except ValueError:
            raise bad("unexpected line %r in the \\data\\ section" % ln)
        if m != len(counts) + 1 or cnt < 0:
            raise bad("orders must be listed as 1, 2, ... (line %r)" % ln)
        counts.append(cnt)
    if not 1 <= len(counts) <= MAX_ORDER:
        raise bad("order %d is outside 1 to %d" % (len(counts), MAX_ORDER))
    words, word_id, ids, logp, backoff = [], {}, [], [], []
    for m in range(1, len(counts) + 1):
        while pos < len(lines) and not lines[pos].strip():
            pos += 1
        if pos >= len(lines) or lines[pos].strip() != "\\%d-grams:" % m:
            raise bad("section \\%d-grams: is missing" % m)
        pos += 1
        rows, ps, bs = [], [], []
        while pos < len(lines) and not lines[pos].startswith("\\"):
            ln = lines[pos].strip()
            pos += 1
            if not ln:
                continue
            f = ln.split()
            if len(f) not in (m + 1, m + 2):
                raise bad("line %r does not hold a %d-gram" % (ln, m))
            try:
                p = float(f[0])
                b = float(f[m + 1]) if len(f) == m + 2 else 0.0
            except ValueError:
                raise bad("line %r does not hold a %d-gram" % (ln, m))
            if m == 1:
                if f[1] in word_id:
                    raise bad("word %r is listed twice" % f[1])
                word_id[f[1]] = len(words)
                words.append(f[1])
            try:
                rows.append([word_id[w] for w in f[1:m + 1]])
            except KeyError:
                raise bad("line %r names a word that is no unigram" % ln)
            ps.append(p)
            bs.append(b)
        if len(rows) != counts[m - 1]:
            raise bad("section \\%d-grams: holds %d entries, the header says %d" % (m, len(rows), counts[m - 1]))
        ids.append(np.array(rows, np.int32).reshape(len(rows), m))
        logp.append(np.array(ps, np.float32))
        backoff.append(np.array(bs, np.float32))
    while pos < len(lines) and not lines[pos].strip():
        pos += 1
    if pos >= len(lines) or lines[pos].strip() != "\\end\\":
        raise bad("the \\end\\ mark is missing")
    if "<s>" not in word_id:
        raise bad("it has no <s> unigram")
    return ArpaLM(words, ids, logp, backoff, counts)


def make_table(keys, values, what="table", spread=1):
    """Open-addressing table of shape (slots, 2) int64 [key, value] from uint64 keys and int64-representable values: slots = the
    power of two >= 2 * len(keys) (>= 2), times spread (a power of two: load <= 1 / (2 * spread)), linear probing from
    slot_of(key).  ValueError if two keys are equal or one is EMPTY_KEY."""
    keys = np.asarray(keys, np.uint64).reshape(-1)
    values = np.asarray(values).reshape(-1)
    assert len(keys) == len(values)
    if len(np.unique(keys)) != len(keys):
        raise ValueError("%s: two entries have the same hash key; lookups would not be exact" % what)
    if (keys == np.uint64(EMPTY_KEY)).any():
        raise ValueError("%s: an entry hashes to the free-slot mark" % what)
    slots = 2
    while slots < 2 * len(keys):
        slots *= 2
    assert spread >= 1 and spread & (spread - 1) == 0, spread
    slots *= spread
    mask = np.uint64(slots - 1)
    tk = np.full(slots, EMPTY_KEY, np.uint64)
    tv = np.zeros(slots, np.uint64)
    vals = values.astype(np.int64).view(np.uint64) if values.dtype != np.uint64 else values
    pend = np.arange(len(keys))
    slot = (keys ^ (keys >> np.uint64(32))) & mask
    while len(pend):
        s = slot[pend]
        free = tk[s] == np.uint64(EMPTY_KEY)
        # of the pending entries that see a free slot, the first per slot takes it
        cand = pend[free]
        _, first = np.unique(s[free], return_index=True)
        win = cand[first]
        tk[slot[win]] = keys[win]
        tv[slot[win]] = vals[win]
        placed = np.zeros(len(keys), bool)
        placed[win] = True
        pend = pend[~placed[pend]]
        slot[pend] = (slot[pend] + np.uint64(1)) & mask
    return np.stack([tk, tv], axis=1).view(np.int64)


def table_find(table, key):
    """Host-side lookup with the kernel's probe sequence: the value word (as a Python int, unsigned) or None."""
    t = table.view(np.uint64)
    mask = len(t) - 1
    slot = slot_of(int(key), mask)
    for _ in range(len(t)):
        k = int(t[slot, 0])
        if k == int(key):
            return int(t[slot, 1])
        if k == EMPTY_KEY:
            return None
        slot = (slot + 1) & mask
    return None


def word_lookup(table, key):
    v = table_find(table, key)
    return WORD_ABSENT if v is None else (v - (1 << 64) if v >> 63 else v)


def ngram_lookup(table, key):
    """(log10 p, log10 backoff) as fp32, or None."""
    v = table_find(table, key)
    if v is None:
        return None
    pb = np.array([v & 0xffffffff, v >> 32], np.uint32).view(np.float32)
    return pb[0], pb[1]


def word_prefixes(lm, labels, blank, space):
    """{hash of the label string: word id or WORD_PREFIX} over every non-empty prefix of every word that the labels spell.
    ValueError if two different prefixes (or a prefix and the empty string) have the same hash."""
    index = {c: i for i, c in enumerate(labels) if i != blank and i != space}
    out, spelled = {}, {HASH_EMPTY: ""}
    for wid, w in enumerate(lm.words):
        if not w or any(ch not in index for ch in w):
            continue
        h = HASH_EMPTY
        for n, ch in enumerate(w):
            h = hash_ext(h, index[ch])
            if spelled.setdefault(h, w[:n + 1]) != w[:n + 1]:
                raise ValueError("word table: %r and %r have the same hash key; lookups would not be exact" % (spelled[h], w[:n + 1]))
            if n + 1 == len(w):
                out[h] = wid
            else:
                out.setdefault(h, WORD_PREFIX)
    return out


def _ngram_keys(ids):
    h = np.full(len(ids), NGRAM_SEED, np.uint64)
    for col in range(ids.shape[1] - 1, -1, -1):
        t = (h ^ (ids[:, col].astype(np.int64) + 1).astype(np.uint64)) * np.uint64(NGRAM_MUL)
        h = t ^ (t >> np.uint64(29))
    return h


def build_tables(lm, labels, blank, space):
    """(word table, n-gram table) as int64 arrays of shape (slots, 2)."""
    pre = word_prefixes(lm, labels, blank, space)
    wt = make_table(np.array(list(pre.keys()), np.uint64), np.array(list(pre.values()), np.int64), "word table")
    keys = np.concatenate([_ngram_keys(lm.ids[m]) for m in range(lm.order)])
    pbits = np.concatenate(lm.logp).view(np.uint32).astype(np.uint64)
    bbits = np.concatenate(lm.backoff).view(np.uint32).astype(np.uint64)
    gt = make_table(keys, pbits | (bbits << np.uint64(32)), "n-gram table")
    return wt, gt


# ---- character language models (ds2_beam_decode_clm; DESIGN.md "ds2_beam", character language model) --------------------
SPECIAL_TOKENS = ("<s>", "</s>", "<unk>")


def is_character_based(lm):
    """ctcdecode's test: every unigram other than <s>, </s>, <unk> is one Unicode code point long."""
    return all(len(w) == 1 for w in lm.words if w not in SPECIAL_TOKENS)


def char_ids(lm, labels, blank, space_token=None):
    """int32 [C]: the unigram id of every label (exact string match), -1 where the file has no such unigram and at the blank.
    A label " " is looked up as space_token when that is given (ValueError if it is no unigram) and as " " otherwise, which no
    ARPA file holds: the space is then out of vocabulary."""
    if space_token is not None and space_token not in lm.word_id:
        raise ValueError("space_token %r is no unigram of the language model" % (space_token,))
    ids = np.full(len(labels), -1, np.int32)
    for c, tok in enumerate(labels):
        if c == blank:
            continue
        if tok == " " and space_token is not None:
            tok = space_token
        ids[c] = lm.word_id.get(tok, -1)
    return ids


# The character search looks up, per new candidate, keys of which most are absent (the long n-grams), and an absent key walks to
# a free slot; at load 1/2 that is 2 to 3 dependent rounds in a crowded table, at load 1/8 rarely more than one.  Measured on an
# MI355X (DESIGN.md "ds2_beam", character language model): 153 -> 85 us per time step with an order-5 file.  16 bytes a slot.
CHAR_TABLE_SPREAD = 4


def ngram_table(lm, spread=1):
    """The n-gram table of build_tables on its own, with make_table's spread."""
    keys = np.concatenate([_ngram_keys(lm.ids[m]) for m in range(lm.order)])
    pbits = np.concatenate(lm.logp).view(np.uint32).astype(np.uint64)
    bbits = np.concatenate(lm.backoff).view(np.uint32).astype(np.uint64)
    return make_table(keys, pbits | (bbits << np.uint64(32)), "n-gram table", spread)


def build_char_tables(lm, labels, blank, space_token=None, spread=CHAR_TABLE_SPREAD):
    """(label ids int32 [C], n-gram table int64 (slots, 2)) of a character-mode search; the table has the word mode's layout and
    keys at load <= 1 / (2 * spread)."""
    return char_ids(lm, labels, blank, space_token), ngram_table(lm, spread)
