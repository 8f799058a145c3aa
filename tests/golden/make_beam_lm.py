"""Writes the small ARPA language models of the beam-search tests under tests/golden/lm/:

    toy3.arpa   trigram over about 30 words from the toy corpus below; trigrams seen once are cut, so some are missing
    toy1.arpa   the unigrams of the same corpus
    toy5.arpa   order 5 over five words

    python tests/golden/make_beam_lm.py                     # rewrites the three fixtures
    python tests/golden/make_beam_lm.py --large /tmp/big.arpa [--words 50000 --ngrams 400000]
                                                            # a synthetic trigram for tools/bench_beam.py --lm; not a fixture

The models are backoff models with absolute discounting: a stored n-gram (h, w) has P(w | h) = (count(h w) - D) / count(h .),
and the mass a context h keeps back is spread over the words it has no n-gram for in proportion to the lower-order model:
backoff(h) = (1 - sum of the stored P(w | h)) / (1 - sum over the same w of P(w | h without its first word)).  So every context
sums to one, which tests/test_beam_lm_reference.py checks from the printed values.  Unigrams are add-one-half estimates over the
vocabulary with </s> and <unk>; <s> gets log10 p = -99 as is customary.  Values are printed with DIGITS decimals."""
import argparse
import math
import os

DIGITS = 6
D = 0.5
HERE = os.path.dirname(os.path.abspath(__file__))

CORPUS3 = """
THE CAT SAT ON THE MAT
THE CAT SAT ON THE MAT
THE DOG SAT ON THE MAT
THE DOG RAN
THE CAT RAN
A CAT AND A DOG RAN
A CAT AND A DOG RAN
AN ANT SAT ON A HAT
AN ANT SAT ON A HAT
AN ANT AND A CAT SAT
IT'S A BIG RED HAT
IT'S A BIG RED HAT
IT'S A BIG DOG
IT'S THE RED MAT
HE SAW THE CAT
HE SAW THE CAT
SHE SAW THE DOG
SHE SAW AN ANT
WE SAW A BIG CAT
WE SAW THE BIG RED DOG
THE ANT IS ON THE HAT
THE ANT IS ON THE HAT
THE HAT IS RED
THE HAT IS RED
THE MAT IS BIG
HE RAN AND SHE SAT
HE RAN AND SHE SAT
THEY SAT IN THE TENT
THEY SAT IN THE TENT
THEY RAN TO THE TENT
AT TEN HE ATE A NUT
AT TEN SHE ATE A NUT
AT TEN SHE ATE A NUT
NO ANT ATE THE NUT
TO EAT AT TEN IS NEAT
AN ANT CAN EAT AND A CAT CAN EAT
"""

CORPUS5 = """
A AN A AN A NA
A AN A AN A NA
AN A NAN A ANNA
AN A NAN A ANNA
ANNA AN A NAN A AN
A NA A NA AN ANNA
A NA A NA AN ANNA
NAN A AN A NA A
NA NA NAN
A AN A AN A AN A NA
"""


def build(corpus, order, cutoffs):
    """cutoffs[m]: smallest count of an (m + 1)-gram that is stored.  Returns per order a dict {words tuple: (log10 p, log10 bo or
    None)}, words in first-seen order."""
    sents = [["<s>"] + ln.split() + ["</s>"] for ln in corpus.strip().split("\n")]
    vocab = ["<unk>", "<s>", "</s>"]
    for s in sents:
        for w in s:
            if w not in vocab:
                vocab.append(w)
    cnt = [dict() for _ in range(order)]
    for s in sents:
        for m in range(order):
            for i in range(len(s) - m):
                g = tuple(s[i:i + m + 1])
                cnt[m][g] = cnt[m].get(g, 0) + 1
    # unigrams
    z = sum(cnt[0].get((w,), 0) + 0.5 for w in vocab if w != "<s>")
    prob = [{(w,): (cnt[0].get((w,), 0) + 0.5) / z for w in vocab if w != "<s>"}]
    prob[0][("<s>",)] = 1e-99
    bo = [dict() for _ in range(order)]

    def full(g):
        """P(g[-1] | g[:-1]) of the model built so far"""
        m = len(g) - 1
        if m < len(prob) and g in prob[m]:
            return prob[m][g]
        if m == 0:
            return 0.0
        return bo[m - 1].get(g[:-1], 1.0) * full(g[1:])

    for m in range(1, order):
        total = {}
        for g, c in cnt[m].items():
            total[g[:-1]] = total.get(g[:-1], 0) + c
        prob.append({g: (c - D) / total[g[:-1]] for g, c in cnt[m].items() if c >= cutoffs[m] and g[:-1] in prob[m - 1]})
        kept, lower = {}, {}
        for g, p in prob[m].items():
            kept[g[:-1]] = kept.get(g[:-1], 0.0) + p
        for g in prob[m]:
            lower[g[:-1]] = lower.get(g[:-1], 0.0) + full(g[1:])
        for h in kept:
            bo[m - 1][h] = (1.0 - kept[h]) / (1.0 - lower[h])
    out = []
    for m in range(order):
        keys = sorted(prob[m], key=lambda g: [vocab.index(w) for w in g])
        out.append({g: (math.log10(prob[m][g]), math.log10(bo[m][g]) if g in bo[m] else None) for g in keys})
    return out


def write_arpa(path, model):
    lines = ["\\data\\"] + ["ngram %d=%d" % (m + 1, len(t)) for m, t in enumerate(model)] + [""]
    for m, t in enumerate(model):
        lines.append("\\%d-grams:" % (m + 1))
        for g, (p, b) in t.items():
            row = "%.*f\t%s" % (DIGITS, p, " ".join(g))
            lines.append(row if b is None else row + "\t%.*f" % (DIGITS, b))
        lines.append("")
    lines.append("\\end\\")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def write_large(path, n_words, n_ngrams, seed=0):
    """A synthetic trigram for timing only: random words over A-Z, random bigrams and trigrams with random values (not normalised)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    words, seen = ["<unk>", "<s>", "</s>"], set()
    while len(words) < n_words + 3:
        w = "".join(chr(65 + int(c)) for c in rng.integers(0, 26, size=int(rng.integers(2, 9))))
        if w not in seen:
            seen.add(w)
            words.append(w)
    V = len(words)
    with open(path, "w") as f:
        bi = np.unique(rng.integers(3, V, size=(n_ngrams, 2)), axis=0)
        tri = np.unique(np.concatenate([bi[rng.integers(0, len(bi), size=n_ngrams)], rng.integers(3, V, size=(n_ngrams, 1))], axis=1),
                        axis=0)
        f.write("\\data\\\nngram 1=%d\nngram 2=%d\nngram 3=%d\n\n\\1-grams:\n" % (V, len(bi), len(tri)))
        for w, p, b in zip(words, -rng.uniform(2, 6, V), -rng.uniform(0, 1, V)):
            f.write("%.6f\t%s\t%.6f\n" % (-99 if w == "<s>" else p, w, b))
        f.write("\n\\2-grams:\n")
        for (a, c), p, b in zip(bi, -rng.uniform(0.5, 4, len(bi)), -rng.uniform(0, 1, len(bi))):
            f.write("%.6f\t%s %s\t%.6f\n" % (p, words[a], words[c], b))
        f.write("\n\\3-grams:\n")
        for (a, c, d), p in zip(tri, -rng.uniform(0.2, 3, len(tri))):
            f.write("%.6f\t%s %s %s\n" % (p, words[a], words[c], words[d]))
        f.write("\n\\end\\\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large", default=None)
    ap.add_argument("--words", type=int, default=50000)
    ap.add_argument("--ngrams", type=int, default=400000)
    a = ap.parse_args()
    if a.large:
        write_large(a.large, a.words, a.ngrams)
        return
    out = os.path.join(HERE, "lm")
    os.makedirs(out, exist_ok=True)
    write_arpa(os.path.join(out, "toy3.arpa"), build(CORPUS3, 3, [1, 1, 2]))
    write_arpa(os.path.join(out, "toy1.arpa"), build(CORPUS3, 1, [1]))
    write_arpa(os.path.join(out, "toy5.arpa"), build(CORPUS5, 5, [1, 1, 1, 1, 2]))


if __name__ == "__main__":
    main()
