"""Search of the language-model weights of ``BeamCTCDecoder`` on the device: the reference's ``search_lm_params.py`` runs one
evaluation per (alpha, beta) trial; here every batch is decoded at all points in one launch (``ops.beam_decode_lm_grid``, or
``ops.beam_decode_clm_grid`` for a decoder in character mode) and the
character and word errors of every point's best transcript are counted on the device (``ops.error_counts``), so that per batch no
transcript travels to the host.  ``LMGridSearch.save`` writes the JSON list of ``[alpha, beta, WER, CER]`` that the reference's
``select_lm_params.py`` loads."""
import json

import torch

from . import ops


class LMGridSearch:
    def __init__(self, decoder, points, max_ws_bytes=1 << 30):
        """decoder: a BeamCTCDecoder with lm_path, in word or in character mode (None: points and counters only); points: a
        sequence of (alpha, beta) pairs."""
        self.points = [(float(a), float(b)) for a, b in points]
        if not self.points:
            raise ValueError("LMGridSearch needs at least one (alpha, beta) point")
        if decoder is not None and getattr(decoder, "lm", None) is None:
            raise ValueError("LMGridSearch needs a BeamCTCDecoder with lm_path")
        if decoder is not None and getattr(decoder, "hotwords", None):
            raise ValueError("LMGridSearch does not support hot words: the weight search is not boosted; call "
                             "set_hotwords(None) on the decoder first")
        self.decoder, self.max_ws_bytes = decoder, max_ws_bytes
        self.reset()

    @classmethod
    def from_ranges(cls, alpha_from, alpha_to, n_alpha, beta_from, beta_to, n_beta, decoder=None, **kw):
        """The Cartesian grid of n_alpha x n_beta evenly spaced values, ends included, alpha-major: point a * n_beta + b.
        Without a decoder the object only holds points and counters (set the decoder before update)."""
        return cls(decoder, grid_points(alpha_from, alpha_to, n_alpha, beta_from, beta_to, n_beta), **kw)

    def reset(self):
        # [G] character errors, [G] word errors, reference characters, reference words: int64, on the device from the first update
        self.char_err = self.word_err = self.ref_chars = self.ref_words = None

    def update(self, probs, sizes, targets, target_sizes):
        """One batch: probs (N, T', C) and sizes as for decoder.decode; targets the flat concatenation of the references' labels
        and target_sizes their lengths, as the metric classes take them."""
        if self.decoder is None:
            raise ValueError("LMGridSearch.update needs a decoder")
        G = len(self.points)
        toks, _, lens, _, _ = self.decoder.decode_grid_device(probs, sizes, self.points, self.max_ws_bytes)
        if lens.shape[1] == 0:
            return
        ce, we, rc, rw = ops.error_counts(toks, lens, targets, target_sizes, self.decoder.space_index)
        if self.char_err is None:
            z = lambda n: torch.zeros(n, dtype=torch.int64, device=ce.device)
            self.char_err, self.word_err, self.ref_chars, self.ref_words = z(G), z(G), z(1), z(1)
        self.char_err += ce.view(G, -1).sum(1, dtype=torch.int64)
        self.word_err += we.view(G, -1).sum(1, dtype=torch.int64)
        self.ref_chars += rc.sum(dtype=torch.int64)
        self.ref_words += rw.sum(dtype=torch.int64)

    def _counts(self):
        G = len(self.points)
        if self.char_err is None:
            return [0] * G, [0] * G, 0, 0
        as_list = lambda t: [int(v) for v in torch.as_tensor(t).reshape(-1).tolist()]
        return as_list(self.char_err), as_list(self.word_err), as_list(self.ref_chars)[0], as_list(self.ref_words)[0]

    def results(self):
        """[[alpha, beta, WER, CER], ...] in percent, in the order of the points; the rates as decoder._ErrorRate.compute forms
        them."""
        ce, we, chars, words = self._counts()
        return [[a, b, float(we[g]) / max(words, 1) * 100, float(ce[g]) / max(chars, 1) * 100]
                for g, (a, b) in enumerate(self.points)]

    def best(self, metric="wer"):
        """The [alpha, beta, WER, CER] row with the lowest WER (metric="wer") or CER ("cer"); of equal rows the first point."""
        if metric not in ("wer", "cer"):
            raise ValueError("metric must be 'wer' or 'cer', got %r" % (metric,))
        col = 2 if metric == "wer" else 3
        rows = self.results()
        return min(rows, key=lambda r: r[col])     # min keeps the first of equal keys

    def save(self, path):
        with open(path, "w") as f:
            json.dump(self.results(), f)


def grid_points(alpha_from, alpha_to, n_alpha, beta_from, beta_to, n_beta):
    n_alpha, n_beta = int(n_alpha), int(n_beta)
    if n_alpha < 1 or n_beta < 1:
        raise ValueError("n_alpha and n_beta must be at least 1, got %d and %d" % (n_alpha, n_beta))
    line = lambda lo, hi, n: [float(lo) + (float(hi) - float(lo)) * i / (n - 1) if n > 1 else float(lo) for i in range(n)]
    return [(a, b) for a in line(alpha_from, alpha_to, n_alpha) for b in line(beta_from, beta_to, n_beta)]
