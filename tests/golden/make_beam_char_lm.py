"""Writes the small character n-gram models of the character-LM beam-search tests under tests/golden/lm/:

    char1.arpa, char3.arpa, char5.arpa   orders 1, 3 and 5 over the English label set, from the sentences that
                                         tests/test_gpu_beam_lm.py plants (each repeated a seeded number of times); the space is
                                         written as the token "|", and the labels that the sentences do not use (J, K, L, P, Q,
                                         ...) are absent from the files
    cjk3.arpa                            order 3 over 300 code points from U+4E00, no space at all, from seeded random sentences
                                         of a sparse Markov chain

    python tests/golden/make_beam_char_lm.py

Every unigram is one code point long, so lm.is_character_based holds for all four.  The estimator is make_beam_lm.build (absolute
discounting, every context sums to one); higher orders are cut at a count of 2, so some n-grams are missing and the search backs
off.  Nothing here is drawn from real text."""
import os

import numpy as np

from make_beam_lm import DIGITS, build

HERE = os.path.dirname(os.path.abspath(__file__))
SPACE_TOKEN = "|"
SENTENCES = ["THE CAT SAT ON THE MAT", "IT'S A BIG RED HAT", "AN ANT AND A CAT SAT", "HE SAW THE DOG", "A CAT AND A DOG RAN",
             "THEY SAT IN THE TENT", "AT TEN SHE ATE A NUT", "THE HAT IS RED"]
CJK_BASE, CJK_COUNT = 0x4E00, 300


def english_corpus(seed=0):
    """the sentences as lines of one-character tokens, the space as SPACE_TOKEN"""
    rng = np.random.default_rng(seed)
    lines = []
    for s in SENTENCES:
        lines += [" ".join(SPACE_TOKEN if ch == " " else ch for ch in s)] * int(rng.integers(1, 4))
    return "\n".join(lines)


def cjk_chars():
    return [chr(CJK_BASE + i) for i in range(CJK_COUNT)]


def cjk_corpus(seed=1, sentences=150):
    """every code point once (in runs of ten), then sentences of a Markov chain in which a character has three likely successors"""
    rng = np.random.default_rng(seed)
    ch = cjk_chars()
    lines = [" ".join(ch[i:i + 10]) for i in range(0, CJK_COUNT, 10)]
    succ = rng.integers(0, CJK_COUNT, size=(CJK_COUNT, 3))
    for _ in range(sentences):
        c = int(rng.integers(0, 40))                     # sentences start in a small set, so that starts repeat
        line = [c]
        for _ in range(int(rng.integers(3, 10))):
            c = int(succ[c, int(rng.integers(0, 3))]) if rng.random() < 0.9 else int(rng.integers(0, CJK_COUNT))
            line.append(c)
        lines.append(" ".join(ch[i] for i in line))
    return "\n".join(lines)


def write_arpa(path, model):
    """make_beam_lm.write_arpa, as UTF-8 whatever the locale"""
    lines = ["\\data\\"] + ["ngram %d=%d" % (m + 1, len(t)) for m, t in enumerate(model)] + [""]
    for m, t in enumerate(model):
        lines.append("\\%d-grams:" % (m + 1))
        for g, (p, b) in t.items():
            row = "%.*f\t%s" % (DIGITS, p, " ".join(g))
            lines.append(row if b is None else row + "\t%.*f" % (DIGITS, b))
        lines.append("")
    lines.append("\\end\\")
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


def main():
    out = os.path.join(HERE, "lm")
    os.makedirs(out, exist_ok=True)
    eng = english_corpus()
    write_arpa(os.path.join(out, "char1.arpa"), build(eng, 1, [1]))
    write_arpa(os.path.join(out, "char3.arpa"), build(eng, 3, [1, 1, 2]))
    write_arpa(os.path.join(out, "char5.arpa"), build(eng, 5, [1, 1, 2, 2, 2]))
    write_arpa(os.path.join(out, "cjk3.arpa"), build(cjk_corpus(), 3, [1, 1, 2]))


if __name__ == "__main__":
    main()
