"""GPU checks of the multi-hypothesis CTC (ds2_ctc_multi_forward / _backward, ops.ctc_multi_forward / _backward): several label
rows per clip against the same frames, one weighted gradient.  References: the existing single-sequence entry bit for bit (one row
per clip, weight 1) and the fp64 oracle per row (tests/mwer_reference.py)."""
import numpy as np
import pytest
import torch

import mwer_reference as R
from fixtures import DEV, cu, np64
from deepspeech.pytorch_amd import mwer, ops
from oracle import ds2_oracle as O

pytestmark = pytest.mark.gpu

NLL_TOL = dict(rtol=2e-5, atol=1e-4)                 # the bar of test_gpu_kernels._ctc_check for a per-sequence nll


def grad_bar(Tp):
    """the bar of test_gpu_kernels._ctc_check for one sequence's gradient (targets of up to 200 labels)"""
    return max(2e-5, 2e-6 * Tp)


def _case(N, Tp, tlens, seed, Cc=29, scale=2.0):
    rs = np.random.RandomState(seed)
    logits = rs.standard_normal((Tp, N, Cc)) * scale
    targets = rs.randint(1, Cc, size=int(np.sum(tlens)))
    if len(targets) > 3:                              # some repeated labels (the s-2 skip rule)
        targets[1] = targets[0]
        targets[-1] = targets[-2]
    return logits, targets


def _dev_logits(logits):
    Tp, N, Cc = logits.shape
    lg = torch.zeros((Tp * N, (Cc + 31) // 32 * 32), dtype=torch.float32, device=DEV)
    lg[:, :Cc] = cu(logits.reshape(Tp * N, Cc))
    return lg


def _dev_rows(hyps):
    rows, lens = mwer.pack_hypotheses(hyps)
    return torch.from_numpy(rows).to(DEV), torch.from_numpy(lens).to(DEV)


def _split(targets, tlens):
    offs = np.concatenate([[0], np.cumsum(tlens)])
    return [targets[offs[i]:offs[i + 1]].tolist() for i in range(len(tlens))]


@pytest.mark.parametrize("recursion", [0, 1])
@pytest.mark.parametrize("N,Tp,lens,tlens,Cc", [
    (3, 31, [31, 25, 19], [7, 6, 4], 29),
    (4, 40, [40, 39, 15, 11], [9, 9, 3, 21], 29),               # the last clip is infeasible
    (4, 130, [130, 129, 121, 9], [63, 64, 57, 4], 29),          # pair tiles: 64 / 65 pairs = one wave / the first pair of a second
    (2, 9, [9, 5], [0, 2], 29),                                 # an empty target
    (3, 31, [31, 25, 19], [7, 6, 4], 257),                      # the _big family (class rows not staged in LDS)
])
def test_one_row_per_clip_has_the_bits_of_the_single_sequence_entry(N, Tp, lens, tlens, Cc, recursion):
    logits, targets = _case(N, Tp, tlens, seed=Tp + N, Cc=Cc)
    lg = _dev_logits(logits)
    offs = np.concatenate([[0], np.cumsum(tlens)[:-1]]).astype(np.int32)
    ild = torch.from_numpy(np.asarray(lens, np.int32)).to(DEV)
    _, nll1, dl1 = ops.ctc_loss_grad(lg, torch.from_numpy(targets.astype(np.int32)).to(DEV), torch.from_numpy(offs).to(DEV), ild,
                                     torch.from_numpy(np.asarray(tlens, np.int32)).to(DEV), Tp, N, Cc, 0, int(max(tlens)),
                                     recursion=recursion)
    rows, rl = _dev_rows([_split(targets, tlens)])
    nll, state = ops.ctc_multi_forward(lg, rows, rl, ild, Tp, N, Cc, 0, want_grad=True, max_target_len=int(max(tlens)),
                                       recursion=recursion)
    dl = ops.ctc_multi_backward(state, torch.ones((1, N), dtype=torch.float32, device=DEV), lg.shape[1])
    inf = torch.isinf(nll[0])
    feasible = [2 * s + 1 <= 2 * t + 1 and s <= t for s, t in zip(tlens, lens)]
    assert inf.tolist() == [not f for f in feasible]              # exactly the infeasible rows (no repeats needed to break these)
    assert torch.all(nll1[inf] == 0)                              # zero_infinity there, +inf here
    assert torch.equal(nll[0][~inf], nll1[~inf])
    assert torch.equal(dl, dl1)


# R = 3, N = 3, T' = 31: rows of different lengths per clip -- repeated labels, an empty row, an absent row, an infeasible row (26
# labels in 25 frames), a clip without frames
SC_LENS = [31, 25, 0]
SC_HYPS = [[[5, 5, 9, 2, 2, 2, 17], [3, 8, 8, 1, 28, 4], [4, 4]],
           [[], None, [7]],
           [[12, 1, 1, 6], [(i % 27) + 1 for i in range(26)], None]]
SC_INF = [[False, False, True], [False, True, True], [False, True, True]]


@pytest.fixture(scope="module")
def score_case():
    rs = np.random.RandomState(31)
    logits = rs.standard_normal((31, 3, 29)) * 2.0
    lp = O.log_softmax(logits)
    nll = np.full((3, 3), np.inf)
    grads = np.zeros((3, 3, 31, 29))
    for r in range(3):
        for n in range(3):
            if SC_HYPS[r][n] is not None:
                nll[r, n], grads[r, n] = R.ctc_row(lp, n, SC_HYPS[r][n], SC_LENS[n])
    return logits, lp, nll, grads


def _score_run(logits, hyps, want_grad, recursion=0):
    lg = _dev_logits(logits)
    rows, rl = _dev_rows(hyps)
    ild = torch.tensor(SC_LENS, dtype=torch.int32, device=DEV)
    return lg, ops.ctc_multi_forward(lg, rows, rl, ild, 31, 3, 29, 0, want_grad=want_grad, recursion=recursion)


@pytest.mark.parametrize("recursion", [0, 1])
def test_scores_against_the_oracle(score_case, recursion):
    logits, _, ref, _ = score_case
    _, (nll, state) = _score_run(logits, SC_HYPS, True, recursion)
    got = np64(nll)
    assert np.isposinf(got).tolist() == SC_INF and np.isposinf(ref).tolist() == SC_INF
    ok = ~np.isinf(ref)
    assert np.allclose(got[ok], ref[ok], **NLL_TOL), (got, ref)
    _, (nll0, none) = _score_run(logits, SC_HYPS, False, recursion)
    assert none is None and torch.equal(nll0, nll)                # forward only: the same bits
    if recursion == 1:
        _, (nllp, _) = _score_run(logits, SC_HYPS, False, 0)
        assert torch.equal(nllp, nll)                             # pair tiles and four waves: the same bits


def test_weighted_gradient_against_the_oracle(score_case):
    logits, lp, _, grads = score_case
    Tp, N, Cc = logits.shape
    w = np.random.RandomState(7).uniform(-2.0, 2.0, (3, 3)).astype(np.float32)
    lg, (nll, state) = _score_run(logits, SC_HYPS, True)
    wd = torch.from_numpy(w).to(DEV)
    dl = ops.ctc_multi_backward(state, wd, lg.shape[1])
    got = np64(dl).reshape(Tp, N, lg.shape[1])
    dlp = np.einsum("rn,rntc->tnc", w.astype(np.float64), grads)
    ref = R.to_logits_grad(lp, dlp)
    for n in range(N):
        alive = [r for r in range(3) if not SC_INF[r][n]]
        bound = sum(abs(float(w[r, n])) for r in alive) * grad_bar(Tp)
        err = np.abs(got[:SC_LENS[n], n, :Cc] - ref[:SC_LENS[n], n]).max() if SC_LENS[n] else 0.0
        assert err <= bound, "clip %d: gradient error %.3e, bound %.3e" % (n, err, bound)
        assert np.all(got[SC_LENS[n]:, n, :] == 0)                # frames past the length: exactly zero
    assert np.all(got[:, :, Cc:] == 0)                            # pad columns: exactly zero
    assert np.abs(got[:, 0, :Cc]).max() > 1e-2                    # and the live clips do have a gradient
    # rows without paths contribute nothing whatever their weight: NaN / inf on the absent and infeasible rows and the dead clip
    wbad = w.copy()
    wbad[1, 1], wbad[2, 1], wbad[0, 2], wbad[2, 2] = np.nan, np.inf, -np.inf, np.nan
    assert torch.equal(ops.ctc_multi_backward(state, torch.from_numpy(wbad).to(DEV), lg.shape[1]), dl)
    # two launches: the same bits
    assert torch.equal(ops.ctc_multi_backward(state, wd, lg.shape[1]), dl)
    _, (nll2, state2) = _score_run(logits, SC_HYPS, True)
    assert torch.equal(nll2, nll) and torch.equal(ops.ctc_multi_backward(state2, wd, lg.shape[1]), dl)


def test_a_clip_does_not_see_the_other_clips_rows(score_case):
    logits, _, _, _ = score_case
    w = torch.from_numpy(np.random.RandomState(7).uniform(-2.0, 2.0, (3, 3)).astype(np.float32)).to(DEV)
    lg, (nll, state) = _score_run(logits, SC_HYPS, True)
    dl = ops.ctc_multi_backward(state, w, lg.shape[1]).view(31, 3, -1)
    other = [[SC_HYPS[0][0], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], [9]], [SC_HYPS[1][0], [2], None], [SC_HYPS[2][0], None, [1, 1]]]
    lg2, (nll2, state2) = _score_run(logits, other, True)
    dl2 = ops.ctc_multi_backward(state2, w, lg.shape[1]).view(31, 3, -1)
    assert torch.equal(nll2[:, 0], nll[:, 0]) and torch.equal(dl2[:, 0], dl[:, 0])
    assert not torch.equal(nll2[:, 1], nll[:, 1]) and not torch.equal(dl2[:, 1], dl[:, 1])


def test_seam_of_the_pair_tiles_inside_one_clip():
    """a 64-label and a 65-label row in the same clip (65 / 66 pairs: one wave, and the first pair of a second), T' = 130"""
    Tp, N, Cc = 130, 2, 29
    rs = np.random.RandomState(130)
    logits = rs.standard_normal((Tp, N, Cc)) * 2.0
    lens = [130, 121]
    hyps = [[rs.randint(1, Cc, 64).tolist(), rs.randint(1, Cc, 3).tolist()], [rs.randint(1, Cc, 65).tolist(), rs.randint(1, Cc, 57).tolist()]]
    w = np.array([[1.5, -0.5], [-1.0, 2.0]], np.float32)
    lp = O.log_softmax(logits)
    lg = _dev_logits(logits)
    rows, rl = _dev_rows(hyps)
    ild = torch.tensor(lens, dtype=torch.int32, device=DEV)
    outs = []
    for recursion in (0, 1):
        nll, state = ops.ctc_multi_forward(lg, rows, rl, ild, Tp, N, Cc, 0, want_grad=True, recursion=recursion)
        outs.append((nll, ops.ctc_multi_backward(state, torch.from_numpy(w).to(DEV), lg.shape[1])))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    got_nll, got = np64(outs[0][0]), np64(outs[0][1]).reshape(Tp, N, -1)
    dlp = np.zeros((Tp, N, Cc))
    for r in range(2):
        for n in range(N):
            ref_nll, g = R.ctc_row(lp, n, hyps[r][n], lens[n])
            assert np.allclose(got_nll[r, n], ref_nll, **NLL_TOL), (r, n, got_nll[r, n], ref_nll)
            dlp[:, n] += float(w[r, n]) * g
    ref = R.to_logits_grad(lp, dlp)
    for n in range(N):
        bound = float(np.abs(w[:, n]).sum()) * grad_bar(Tp)
        err = np.abs(got[:, n, :Cc] - ref[:, n]).max()
        assert err <= bound, "clip %d: gradient error %.3e, bound %.3e" % (n, err, bound)


def test_a_row_longer_than_the_sized_rows_is_treated_as_absent():
    """max_target_len sizes the alpha / beta rows; a longer row must not write past them: it reports +inf and adds nothing"""
    logits, _ = _case(2, 12, [0], seed=3)
    lg = _dev_logits(logits)
    rows, rl = _dev_rows([[[1, 2, 3, 4, 5], [6, 7]], [[3, 3], [1, 2, 3]]])
    ild = torch.tensor([12, 12], dtype=torch.int32, device=DEV)
    for recursion in (0, 1):
        nll, state = ops.ctc_multi_forward(lg, rows, rl, ild, 12, 2, 29, 0, want_grad=True, max_target_len=3, recursion=recursion)
        assert torch.isinf(nll).tolist() == [[True, False], [False, False]]
        dl = ops.ctc_multi_backward(state, torch.ones((2, 2), dtype=torch.float32, device=DEV), lg.shape[1])
        assert bool(torch.isfinite(dl).all())
    with pytest.raises(ValueError):
        ops.ctc_multi_forward(lg, rows, rl, ild, 12, 2, 29, 0, max_target_len=6)
    with pytest.raises(ValueError):
        ops.ctc_multi_forward(lg, rows, rl[:1], ild, 12, 2, 29, 0)
    with pytest.raises(ValueError):
        ops.ctc_multi_forward(lg.cpu(), rows, rl, ild, 12, 2, 29, 0)
    with pytest.raises(ValueError):
        ops.ctc_multi_forward(lg, rows, rl, ild, 12, 2, 29, 0, recursion=2)
