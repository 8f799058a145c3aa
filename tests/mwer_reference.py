"""fp64 numpy restatement of MWER training as include/ds2hip.h states it (ds2_ctc_multi_forward / _backward, ds2_mwer_weights):
per-row CTC from the oracle, ds2_error_counts' two edit distances, the softmax over a clip's hypotheses, risk, weights and the
total gradient with respect to the logits."""
import numpy as np

from oracle import ds2_oracle as O


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[len(b)]


def chars_of(labels, space):
    """the labels other than the space (the metric's replace(' ', ''))"""
    return [int(v) for v in labels if int(v) != space]


def words_of(labels, space):
    """maximal runs of labels other than the space (str.split())"""
    words, cur = [], []
    for v in labels:
        if int(v) == space:
            if cur:
                words.append(tuple(cur))
            cur = []
        else:
            cur.append(int(v))
    if cur:
        words.append(tuple(cur))
    return words


def error_count(hyp, ref, space, unit):
    f = words_of if unit == "word" else chars_of
    return levenshtein(f(hyp, space), f(ref, space))


def ref_units(ref, space, unit):
    return len((words_of if unit == "word" else chars_of)(ref, space))


def ctc_row(lp, n, labels, Ti, blank=0):
    """(nll, d nll / d log_probs [T][C]) of ONE label row against clip n's first Ti frames of lp (T, N, C) log-probabilities;
    nll = +inf and a zero gradient for a row without paths or a clip without frames."""
    T, N, C = lp.shape
    S = len(labels)
    if Ti <= 0:
        return np.inf, np.zeros((T, C))
    fn = O.ctc_loss_and_grad_fast if T > 100 else O.ctc_loss_and_grad
    _, nll, g = fn(lp[:, n:n + 1, :], np.asarray(labels, np.int64), np.asarray([Ti]), np.asarray([S]), blank=blank)
    g = g[:, 0, :]
    # the oracle applies zero_infinity: an infeasible row comes back as loss 0 with a zero gradient
    if not np.any(g) and (float(nll[0]) == 0.0):
        return np.inf, np.zeros((T, C))
    return float(nll[0]), g


def weights_rule(nll, err, ce_weight, has_ref=True):
    """The rule of ds2_mwer_weights in fp64.  nll [K + has_ref][N], err [K][N] (negative = not counted).  Returns (weights, risk [N],
    nll_ref [N], loss, phat [K][N])."""
    nll = np.asarray(nll, np.float64)
    K = nll.shape[0] - int(has_ref)
    N = nll.shape[1]
    err = np.asarray(err, np.int64).reshape(K, N)
    w, phat = np.zeros_like(nll), np.zeros((K, N))
    risk, nll_ref = np.zeros(N), np.zeros(N)
    for n in range(N):
        A = [k for k in range(K) if np.isfinite(nll[k, n]) and err[k, n] >= 0]
        if A:
            smax = max(-nll[k, n] for k in A)
            z = 0.0
            for k in A:
                z += np.exp(-nll[k, n] - smax)
            for k in A:
                phat[k, n] = np.exp(-nll[k, n] - smax) / z
            ebar = 0.0
            for k in A:
                ebar += phat[k, n] * err[k, n]
            risk[n] = ebar
            for k in A:
                w[k, n] = -phat[k, n] * (err[k, n] - ebar)
        if has_ref and np.isfinite(nll[K, n]):
            w[K, n] = ce_weight
            nll_ref[n] = nll[K, n]
    loss = 0.0
    rs = rf = 0.0
    for n in range(N):
        rs += risk[n]
        rf += nll_ref[n]
    loss = rs + ce_weight * rf
    return w, risk, nll_ref, loss, phat


def to_logits_grad(lp, dlp):
    """log-softmax backward: gradient by log-probabilities -> gradient by logits"""
    return dlp - np.exp(lp) * dlp.sum(-1, keepdims=True)


def mwer(logits, lens, hyps, refs, space, unit, ce_weight, blank=0):
    """The whole criterion on fixed hypotheses.  logits (T, N, C) fp64; lens [N] frames; hyps[k][n] = label list or None (absent);
    refs[n] = label list.  Returns dict(loss, risk, nll_ref, nll [K+1][N], err [K][N], phat, weights, dlogits (T, N, C))."""
    T, N, C = logits.shape
    K = len(hyps)
    lp = O.log_softmax(logits)
    nll = np.full((K + 1, N), np.inf)
    grads = [[None] * N for _ in range(K + 1)]
    err = np.full((K, N), -1, np.int64)
    for n in range(N):
        for k in range(K + 1):
            y = refs[n] if k == K else hyps[k][n]
            if y is None:
                grads[k][n] = np.zeros((T, C))
                continue
            nll[k, n], grads[k][n] = ctc_row(lp, n, y, int(lens[n]), blank)
            if k < K:
                err[k, n] = error_count(y, refs[n], space, unit)
    w, risk, nll_ref, loss, phat = weights_rule(nll, err, ce_weight)
    dlp = np.zeros((T, N, C))
    for n in range(N):
        for k in range(K + 1):
            if w[k, n] != 0.0:
                dlp[:, n, :] += w[k, n] * grads[k][n]
    return dict(loss=loss, risk=risk, nll_ref=nll_ref, nll=nll, err=err, phat=phat, weights=w, dlogits=to_logits_grad(lp, dlp))
