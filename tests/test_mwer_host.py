"""Host checks of MWER training: the fp64 restatement (tests/mwer_reference.py) against central differences of its own loss, the
weights rule's edge cases, the rank-major packing helpers of deepspeech.pytorch_amd.mwer on CPU tensors, and every ValueError of
MWERLoss."""
import numpy as np
import pytest
import torch

import mwer_reference as R
from deepspeech.pytorch_amd import mwer
from deepspeech.pytorch_amd.decoder import BeamCTCDecoder

LABELS = ["_", "a", "b", "c", " "]


def test_reference_gradient_matches_central_differences():
    """T' = 9, C = 5, K = 3 with the hypothesis set held fixed: the analytic gradient of the reference against central differences of
    its own loss in fp64, relative error < 1e-6."""
    rs = np.random.RandomState(5)
    T, N, C, space = 9, 2, 5, 4
    logits = rs.standard_normal((T, N, C)) * 1.5
    lens = [9, 7]
    refs = [[1, 4, 2, 3], [2, 2, 4, 1]]
    hyps = [[[1, 4, 2], [2, 4, 1]], [[1, 2, 3], [2, 2, 4, 1]], [[3, 4, 2, 3], [1]]]
    for unit in ("word", "char"):
        out = R.mwer(logits, lens, hyps, refs, space, unit, ce_weight=0.3)
        assert len(set(out["err"][:, 0].tolist())) > 1          # otherwise the risk has no gradient at all
        g, h = out["dlogits"], 1e-5
        num = np.zeros_like(logits)
        for idx in np.ndindex(*logits.shape):
            lp, lm = logits.copy(), logits.copy()
            lp[idx] += h
            lm[idx] -= h
            num[idx] = (R.mwer(lp, lens, hyps, refs, space, unit, 0.3)["loss"] - R.mwer(lm, lens, hyps, refs, space, unit, 0.3)["loss"]) / (2 * h)
        rel = np.abs(g - num).max() / np.abs(num).max()
        assert rel < 1e-6, (unit, rel)
        assert np.all(g[7:, 1] == 0)                             # frames past the clip's length


def test_edit_distances_follow_the_error_count_definitions():
    sp = 4
    assert R.error_count([1, 4, 2, 3], [1, 4, 2, 3], sp, "word") == 0
    assert R.error_count([1, 4, 4, 2, 3, 4], [1, 4, 2, 3], sp, "word") == 0      # runs of spaces split like str.split()
    assert R.error_count([1, 2, 3], [1, 4, 2, 3], sp, "word") == 2               # one word against two
    assert R.error_count([1, 2, 3], [1, 4, 2, 3], sp, "char") == 0               # the spaces are dropped
    assert R.error_count([], [1, 4, 2], sp, "word") == 2 and R.error_count([], [1, 4, 2], sp, "char") == 2
    assert R.ref_units([1, 4, 2, 3], sp, "word") == 2 and R.ref_units([1, 4, 2, 3], sp, "char") == 3


def test_weights_rule_edge_cases():
    inf = np.inf
    # empty A (all absent, or all errors uncounted): risk 0, weights 0; the reference row still takes ce_weight
    w, risk, nref, loss, _ = R.weights_rule([[inf], [inf], [2.5]], [[3], [1]], 0.25)
    assert risk[0] == 0 and np.all(w[:2] == 0) and w[2, 0] == 0.25 and nref[0] == 2.5 and loss == 0.25 * 2.5
    w, risk, _, _, _ = R.weights_rule([[1.0], [2.0], [2.5]], [[-1], [-1]], 0.25)
    assert risk[0] == 0 and np.all(w[:2] == 0)
    # K = 1: phat = 1, err - ebar = 0
    w, risk, _, loss, phat = R.weights_rule([[7.0], [2.0]], [[5]], 0.0)
    assert w[0, 0] == 0 and risk[0] == 5 and phat[0, 0] == 1 and loss == 5
    # infinite reference: zero_infinity
    w, risk, nref, loss, _ = R.weights_rule([[1.0], [1.0], [inf]], [[0], [2]], 0.5)
    assert w[2, 0] == 0 and nref[0] == 0 and risk[0] == 1.0 and loss == 1.0
    assert w[0, 0] == 0.5 and w[1, 0] == -0.5                   # -phat (err - ebar) with phat = 1/2, ebar = 1
    # the weights of a clip sum to zero: the risk does not move when every score shifts alike
    rs = np.random.RandomState(1)
    w, _, _, _, _ = R.weights_rule(np.abs(rs.standard_normal((5, 3))) * 4, rs.randint(0, 6, (4, 3)), 0.0)
    assert np.abs(w[:4].sum(0)).max() < 1e-15


def test_rank_major_packing_on_cpu_tensors():
    N, B, ld = 3, 4, 5
    tokens = torch.arange(N * B * ld, dtype=torch.int32).view(N, B, ld)
    lens = torch.tensor([[5, 4, 3, 2], [1, 0, 0, 0], [2, 2, 0, 0]], dtype=torch.int32)
    scores = torch.tensor([[1.0, 2.0, 3.0, 4.0], [0.5, float("inf"), float("inf"), float("inf")], [1.0, 1.5, float("inf"), float("inf")]])
    tk, ln = mwer.rank_major(tokens, lens, scores, 3)
    assert tk.shape == (3, N, ld) and ln.shape == (3, N) and tk.is_contiguous() and ln.is_contiguous()
    for r in range(3):
        for n in range(N):
            assert torch.equal(tk[r, n], tokens[n, r])
    assert ln.tolist() == [[5, 1, 2], [4, -1, 2], [3, -1, -1]]
    with pytest.raises(ValueError):
        mwer.rank_major(tokens, lens, scores, 5)
    # the reference joins as rank K; the width cuts the padding and widens short buffers
    ref_rows, ref_lens = mwer.pad_rows(torch.tensor([1, 2, 3, 1, 2, 2, 2, 2, 2, 2, 2]), torch.tensor([3, 0, 8]))
    assert ref_rows.shape == (3, 8) and ref_lens.tolist() == [3, 0, 8]
    assert ref_rows[0].tolist() == [1, 2, 3, 0, 0, 0, 0, 0] and ref_rows[2].tolist() == [1] + [2] * 7
    rows, all_lens = mwer.append_rank(tk, ln, torch.from_numpy(ref_rows), torch.from_numpy(ref_lens), 8)
    assert rows.shape == (4, N, 8) and all_lens.tolist() == ln.tolist() + [[3, 0, 8]]
    assert torch.equal(rows[:3, :, :5], tk) and torch.all(rows[:3, :, 5:] == 0) and torch.equal(rows[3], torch.from_numpy(ref_rows))
    rows, _ = mwer.append_rank(tk, ln, torch.from_numpy(ref_rows), torch.from_numpy(ref_lens), 4)
    assert rows.shape == (4, N, 4) and torch.equal(rows[:3], tk[:, :, :4])
    rows, all_lens = mwer.append_rank(tk[:0], ln[:0], torch.from_numpy(ref_rows), torch.from_numpy(ref_lens), 8)     # nbest = 0
    assert rows.shape == (1, N, 8) and all_lens.tolist() == [[3, 0, 8]]
    with pytest.raises(ValueError):
        mwer.pad_rows(torch.tensor([1, 2]), torch.tensor([3]))
    hr, hl = mwer.pack_hypotheses([[[1, 2], None, []], [[3], [1, 1, 1], None]])
    assert hr.shape == (2, 3, 3) and hl.tolist() == [[2, -1, 0], [1, 3, -1]] and hr[1, 1].tolist() == [1, 1, 1]
    with pytest.raises(ValueError):
        mwer.pack_hypotheses([[[1]], [[1], [2]]])


def test_mwer_loss_value_errors():
    dec = BeamCTCDecoder(LABELS, beam_width=8, blank_index=0)
    for bad in (-1, 9, 2.5):
        with pytest.raises(ValueError):
            mwer.MWERLoss(dec, nbest=bad)
    with pytest.raises(ValueError):
        mwer.MWERLoss(dec, unit="phone")
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            mwer.MWERLoss(dec, ce_weight=bad)
    with pytest.raises(ValueError):
        mwer.MWERLoss(dec, nbest=0, ce_weight=0.0)
    crit = mwer.MWERLoss(dec, nbest=8, ce_weight=0.0, unit="char")
    assert crit.blank == 0 and crit.last is None
    with pytest.raises(ValueError):                              # a host tensor: there is no CPU fallback
        crit(torch.zeros(6, 2, 5), torch.tensor([1, 2, 3]), torch.tensor([6, 6]), torch.tensor([2, 1]))
    with pytest.raises(ValueError):
        crit.from_logits(torch.zeros(12, 32), torch.tensor([1, 2, 3]), torch.tensor([6, 6]), torch.tensor([2, 1]), 2, 6, 5, 0)
    with pytest.raises(ValueError):
        mwer.ctc_scores(torch.zeros(6, 2, 5), torch.tensor([6, 6]), [[[1], [2]]])
    with pytest.raises(ValueError):
        crit.expected_error_rate()
    with pytest.raises(ValueError):
        dec.nbest_device(torch.zeros(2, 6, 5), None, 2)
    mwer.MWERLoss(dec, nbest=0, ce_weight=1.0)                   # plain CTC through the new path
