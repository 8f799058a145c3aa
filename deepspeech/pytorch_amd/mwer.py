"""Minimum word error rate training (Prabhavalkar et al. 2018) with the decoder inside the training step, on the device.

``MWERLoss`` decodes the K best hypotheses of every clip with the current weights (BeamCTCDecoder.nbest_device), counts their
errors against the reference (ds2_error_counts), scores every hypothesis and the reference exactly with one multi-hypothesis CTC
call (ds2_ctc_multi_forward), turns likelihoods and error counts into weights (ds2_mwer_weights; the rule is stated in
include/ds2hip.h and DESIGN.md) and lets ds2_ctc_multi_backward write the one gradient:

    loss = sum_n sum_k phat_k err_k  +  ce_weight * sum_n -log p(reference_n | x_n)

``ctc_scores`` is the forward half alone: the exact full-sum CTC -log p(y | x) of arbitrary label rows, e.g. to rescore an n-best
list (the beam search's own score sums only the paths its beam kept).

Rows are rank-major throughout, row r * N + n = rank r of clip n, the convention of ds2_error_counts.  There is no CPU fallback.
"""
import math

import numpy as np
import torch

from . import ops

UNITS = ("word", "char")
_STAGING = ops.PinnedRing()        # the reference rows of a step: one pinned slot, one in-stream copy (see ops.PinnedRing)


def rank_major(tokens, lens, scores, nbest):
    """The best `nbest` ranks of a search's outputs, clip-major as _beam_outputs leaves them -- tokens (N, B, ld), lens (N, B),
    scores (N, B) -- as rank-major rows: (tokens [nbest][N][ld] int32, lens [nbest][N] int32), lens = -1 where the score is +inf (no
    beam alive at that rank).  Plain torch: works on host tensors too."""
    K = int(nbest)
    if not 1 <= K <= tokens.shape[1]:
        raise ValueError("nbest must be in [1, %d], got %r" % (tokens.shape[1], nbest))
    tk = tokens[:, :K].permute(1, 0, 2).contiguous().to(torch.int32)
    ln = lens[:, :K].t().to(torch.int32)
    dead = torch.isinf(scores[:, :K].t()) & (scores[:, :K].t() > 0)
    return tk, torch.where(dead, torch.full_like(ln, -1), ln).contiguous()


def pad_rows(flat, sizes, width=None):
    """Flat concatenated labels + their N sizes -> host numpy (rows [N][width] int32, zero-padded; sizes [N] int32); width
    defaults to the longest row (at least 1)."""
    sz = np.asarray(torch.as_tensor(sizes).cpu()).astype(np.int64).reshape(-1)
    fl = np.asarray(torch.as_tensor(flat).cpu()).astype(np.int32).reshape(-1)
    if (sz < 0).any() or int(sz.sum()) > fl.size:
        raise ValueError("sizes add up to %d labels, the flat array has %d" % (int(sz.sum()), fl.size))
    longest = int(sz.max()) if sz.size else 0
    width = max(longest, 1) if width is None else int(width)
    if width < longest:
        raise ValueError("a row has %d labels, the width is %d" % (longest, width))
    rows = np.zeros((sz.size, width), np.int32)
    o = 0
    for n, s in enumerate(sz):
        rows[n, :s] = fl[o:o + s]
        o += int(s)
    return rows, sz.astype(np.int32)


def pack_hypotheses(hyps):
    """A list [R] of lists [N] of label lists (None = the row is absent) -> host numpy (rows [R][N][ld] int32, lens [R][N] int32 with
    -1 for absent rows)."""
    R = len(hyps)
    N = len(hyps[0]) if R else 0
    if R < 1 or N < 1 or any(len(h) != N for h in hyps):
        raise ValueError("hypotheses must be a non-empty list of ranks, each a list of one label list per clip")
    ld = max([len(y) for h in hyps for y in h if y is not None] + [1])
    rows, lens = np.zeros((R, N, ld), np.int32), np.full((R, N), -1, np.int32)
    for r, h in enumerate(hyps):
        for n, y in enumerate(h):
            if y is not None:
                rows[r, n, :len(y)] = np.asarray(y, np.int32)
                lens[r, n] = len(y)
    return rows, lens


def append_rank(tokens, lens, row, row_lens, width):
    """Rank-major rows tokens [K][N][ld], lens [K][N] plus one more rank (row [N][lr], row_lens [N]) -> ([K+1][N][width], [K+1][N]);
    labels beyond `width` are cut (the caller passes the longest length in use), missing columns are zero.  Plain torch."""
    K, N = lens.shape
    out = torch.zeros((K + 1, N, max(int(width), 1)), dtype=torch.int32, device=row.device)
    w = min(out.shape[2], tokens.shape[2]) if K else 0
    if w:
        out[:K, :, :w] = tokens[:, :, :w]
    w = min(out.shape[2], row.shape[1])
    out[K, :, :w] = row[:, :w]
    return out, torch.cat([lens.to(torch.int32), row_lens.to(torch.int32).reshape(1, N)], 0)


def _padded_logits(out):
    """(T', N, C) logits or log-probabilities -> [T'*N][C rounded up to 32] f32, as CTCLossHip pads them"""
    Tp, N, Cc = out.shape
    x = torch.zeros((Tp * N, (Cc + 31) // 32 * 32), dtype=torch.float32, device=out.device)
    x[:, :Cc] = out.reshape(Tp * N, Cc).float()
    return x


@torch.no_grad()
def ctc_scores(out, sizes, hypotheses, blank=0):
    """Exact -log p(y | x) of given label rows, forward only (ds2_ctc_multi_forward): every path of y, not only those a beam kept.
    out: (T', N, C) HIP tensor of logits or log-probabilities, as CTCLossHip takes them; sizes [N] frames per clip.
    hypotheses: a pair (tokens [R][N][ld] device int tensor, lens [R][N], negative = absent), e.g. nbest_device's, or a list [R] of
    lists [N] of label lists (None = absent).  Returns nll [R][N] f32 on the device; +inf for absent and infeasible rows.  One scalar
    (the longest row) is read back for rows that live on the device: it picks the recursion's width."""
    if not (torch.is_tensor(out) and out.is_cuda and out.dim() == 3):
        raise ValueError("ctc_scores needs a HIP device tensor (T', N, C); there is no CPU fallback")
    Tp, N, Cc = out.shape
    dev = out.device
    if isinstance(hypotheses, (tuple, list)) and len(hypotheses) == 2 and torch.is_tensor(hypotheses[0]):
        rows, lens = hypotheses
        lens = torch.as_tensor(lens).to(dev, torch.int32)
        longest = max(int(lens.max()), 0)
    else:
        rows_h, lens_h = pack_hypotheses(hypotheses)
        rows, lens, longest = torch.from_numpy(rows_h).to(dev), torch.from_numpy(lens_h).to(dev), int(max(lens_h.max(), 0))
    if rows.dim() != 3 or rows.shape[1] != N:
        raise ValueError("hypotheses has shape %s for %d clips" % (tuple(rows.shape), N))
    nll, _ = ops.ctc_multi_forward(_padded_logits(out), rows.to(dev), lens, torch.as_tensor(sizes).to(dev, torch.int32), Tp, N, Cc,
                                   blank, want_grad=False, max_target_len=min(longest, rows.shape[2]))
    return nll


class _MwerFn(torch.autograd.Function):
    """MWERLoss on padded logits [Tp*N][ld]: like model._CtcFn, the gradient is made in forward for a unit upstream gradient and
    scaled in place by the one backward."""

    @staticmethod
    def forward(ctx, logits, crit, targets, out_lens_dev, target_sizes, N, Tp, Cc, blank):
        dl, loss = crit._forward(logits.detach(), targets, out_lens_dev, target_sizes, N, Tp, Cc, blank)
        ctx.save_for_backward(dl)
        ctx.consumed = False
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        if ctx.consumed:
            raise RuntimeError("DeepSpeech (gfx950): backward through the MWER loss a second time -- its gradient buffer was scaled in "
                               "place by the first backward; run the forward again (retain_graph is not supported)")
        ctx.consumed = True
        return (ops.scale_by_(dl, g.detach().float()),) + (None,) * 8


class MWERLoss:
    """Expected error count over the decoder's n-best list, interpolated with CTC (module docstring; DESIGN.md "MWER training").

    decoder: a BeamCTCDecoder (any configuration: plain, LM, character LM, hot words; only its label rows are used, its LM and
    hot-word terms do not enter the weights).  nbest: hypotheses per clip, 0 .. decoder.beam_width; 0 skips the search and is plain
    CTC through the multi-hypothesis path.  ce_weight: weight of -log p(reference); unit: the errors that are counted, "word" or
    "char" (ds2_error_counts' two counts).  blank: default the decoder's.

    Called as CTCLossHip is, ``loss(out (T',N,C), targets, output_sizes, target_sizes)``, or on the training step's padded logits,
    ``loss.from_logits(logits [T'*N][ld], targets, lens_dev, target_sizes, N, Tp, Cc, blank)`` (the arguments of _CtcFn.apply;
    DeepSpeech.attach_training_loss routes training_step there).  Differentiable with respect to the logits; one backward per
    forward.  The host does nothing between logits and gradient but read ONE scalar, the longest hypothesis, which sizes the
    alpha / beta workspace (ops.error_counts reads its own for the same reason); the reference rows travel as _CtcFn's do.

    After a call ``last`` holds device tensors: risk [N], nll_ref [N], errors [K][N] (-1 for absent ranks), ref_units [N] (None when
    nbest = 0), posterior [K][N] (the renormalised likelihoods phat) and nll [K+1][N]."""

    def __init__(self, decoder, nbest=4, ce_weight=0.01, unit="word", blank=None):
        if unit not in UNITS:
            raise ValueError("unit must be 'word' or 'char', got %r" % (unit,))
        if isinstance(nbest, bool) or int(nbest) != nbest or not 0 <= int(nbest) <= int(decoder.beam_width):
            raise ValueError("nbest must be an integer in [0, beam_width=%d], got %r" % (decoder.beam_width, nbest))
        ce_weight = float(ce_weight)
        if not (math.isfinite(ce_weight) and 0.0 <= ce_weight <= 3.4e38):
            raise ValueError("ce_weight must be a finite value >= 0, got %r" % (ce_weight,))
        if int(nbest) == 0 and ce_weight == 0.0:
            raise ValueError("nbest = 0 with ce_weight = 0 leaves no loss")
        self.decoder, self.nbest, self.ce_weight, self.unit = decoder, int(nbest), ce_weight, unit
        self.blank = decoder.blank_index if blank is None else int(blank)
        self._raw = self._last = None

    def __call__(self, out, targets, output_sizes, target_sizes):
        if not (torch.is_tensor(out) and out.is_cuda):
            raise ValueError("MWERLoss needs a HIP tensor; there is no CPU fallback")
        Tp, N, Cc = out.shape
        return self.from_logits(_padded_logits(out), targets, torch.as_tensor(output_sizes).to(out.device, torch.int32), target_sizes,
                                N, Tp, Cc, self.blank)

    forward = __call__

    def from_logits(self, logits, targets, out_lens_dev, target_sizes, N, Tp, Cc, blank):
        if not (torch.is_tensor(logits) and logits.is_cuda):
            raise ValueError("MWERLoss needs a HIP tensor; there is no CPU fallback")
        return _MwerFn.apply(logits, self, targets, out_lens_dev, target_sizes, N, Tp, Cc, blank)

    @torch.no_grad()
    def _forward(self, logits, targets, out_lens_dev, target_sizes, N, Tp, Cc, blank):
        dev, K = logits.device, self.nbest
        ref_h, rsz_h = pad_rows(targets, target_sizes)
        lr = ref_h.shape[1]
        meta = _STAGING.stage(dev, [rsz_h, ref_h.reshape(-1)])
        rsz, ref = meta[:N], meta[N:].view(N, lr)
        longest_ref = int(rsz_h.max()) if N else 0
        err = units = None
        toks = torch.zeros((0, N, 1), dtype=torch.int32, device=dev)
        lens = torch.zeros((0, N), dtype=torch.int32, device=dev)
        width = longest_ref
        if K:
            probs = ops.softmax_rows(logits, Cc).view(Tp, N, Cc).transpose(0, 1)
            toks, lens = self.decoder.nbest_device(probs, out_lens_dev, K)
            ce, we, rc, rw = ops.error_counts(toks, lens.clamp(min=0), torch.as_tensor(targets).reshape(-1), torch.as_tensor(target_sizes),
                                              self.decoder.space_index)
            err, units = (we, rw) if self.unit == "word" else (ce, rc)
            err = torch.where(lens.reshape(-1) < 0, torch.full_like(err, -1), err)
            width = max(width, int(lens.max()))            # the one scalar read: sizes the alpha / beta rows
        rows, all_lens = append_rank(toks, lens, ref, rsz, width)
        nll, state = ops.ctc_multi_forward(logits, rows, all_lens, out_lens_dev, Tp, N, Cc, blank, want_grad=True,
                                           max_target_len=min(width, rows.shape[2]))
        weights, risk, nll_ref, loss = ops.mwer_weights(nll, err, K, True, self.ce_weight)
        dl = ops.ctc_multi_backward(state, weights, logits.shape[1])
        self._raw = dict(risk=risk, nll_ref=nll_ref, nll=nll, errors=None if err is None else err.view(K, N), ref_units=units)
        self._last = None
        return dl, loss

    @property
    def last(self):
        """the device tensors of the last call (class docstring); posterior is computed on first access"""
        if self._raw is None:
            return None
        if self._last is None:
            r, K = self._raw, self.nbest
            N = r["risk"].shape[0]
            errors = r["errors"] if K else torch.zeros((0, N), dtype=torch.int32, device=r["risk"].device)
            s = -r["nll"][:K]
            s = torch.where(torch.isfinite(s) & (errors >= 0), s, torch.full_like(s, -float("inf")))
            post = torch.nan_to_num(torch.softmax(s, 0), nan=0.0) if K else s
            self._last = dict(risk=r["risk"], nll_ref=r["nll_ref"], errors=errors, ref_units=r["ref_units"], posterior=post, nll=r["nll"])
        return self._last

    def expected_error_rate(self):
        """sum(risk) / sum(ref_units) of the last call, as a float: the expected word (or character) error rate over the n-best
        lists.  Reading it synchronises."""
        if self._raw is None or self._raw["ref_units"] is None:
            raise ValueError("expected_error_rate needs a call with nbest > 0 first")
        return float(self._raw["risk"].double().sum().item()) / max(float(self._raw["ref_units"].sum().item()), 1.0)
