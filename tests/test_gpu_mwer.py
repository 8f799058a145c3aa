"""GPU checks of MWER training (ds2_mwer_weights, mwer.MWERLoss, mwer.ctc_scores, BeamCTCDecoder.nbest_device,
DeepSpeech.attach_training_loss) against the fp64 restatement tests/mwer_reference.py."""
import numpy as np
import pytest
import torch

import mwer_reference as R
from fixtures import DEV, cu, np64
from deepspeech.pytorch_amd import configs, mwer, ops, synth
from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
from deepspeech.pytorch_amd.model import CTCLossHip, DeepSpeech

pytestmark = pytest.mark.gpu

LABELS = configs.LABELS                               # 29 classes: blank 0, the space last
SPACE = LABELS.index(" ")
NLL_TOL = dict(rtol=2e-5, atol=1e-4)                  # the existing bar for a per-sequence nll (test_gpu_kernels._ctc_check)


def grad_bar(Tp):
    return max(2e-5, 2e-6 * Tp)                       # the existing bar for one sequence's gradient


def _ulps(a, b):
    """distance in fp32 units in the last place, +0 and -0 being one value"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


# ---- ds2_mwer_weights alone -------------------------------------------------------------------------------------------------
def _weights_inputs():
    inf = np.inf
    rs = np.random.RandomState(4)
    # clips: all absent | one alive | equal scores | scores 200 apart | random, one error count not counted
    nll = np.array([[inf, 12.5, 7.25, 3.0, 0], [inf, inf, 7.25, 203.0, 0], [inf, inf, 7.25, 403.0, 0], [inf, inf, 7.25, 603.0, 0],
                    [4.0, 9.0, inf, 55.5, 0]], np.float32)
    nll[:, 4] = (np.abs(rs.standard_normal(5)) * 3 + 20).astype(np.float32)
    err = np.array([[1, 3, 0, 2, 4], [2, 0, 1, 7, 1], [0, 0, 5, 1, -1], [9, 1, 2, 0, 6]], np.int32)
    return nll, err


@pytest.mark.parametrize("has_ref", [True, False])
def test_mwer_weights_kernel_against_fp64(has_ref):
    nll, err = _weights_inputs()
    K, N = 4, 5
    ce = float(np.float32(0.3))
    nll = nll if has_ref else nll[:K]
    w, risk, nref, loss = ops.mwer_weights(cu(nll), torch.from_numpy(err).to(DEV), K, has_ref, ce)
    rw, rrisk, rnref, rloss, _ = R.weights_rule(nll.astype(np.float64), err, ce, has_ref)
    for name, got, ref in (("weights", w, rw), ("risk", risk, rrisk), ("nll_ref", nref, rnref)):
        d = _ulps(got.cpu().numpy(), ref.astype(np.float32))
        assert d.max() <= 1, (name, got.cpu().numpy(), ref)
    assert abs(float(loss.item()) - rloss) <= 1e-6 * abs(rloss), (float(loss.item()), rloss)
    got = w.cpu().numpy()
    assert np.all(got[:K, 0] == 0) and float(risk[0]) == 0          # all absent
    assert np.all(got[:K, 1] == 0) and float(risk[1]) == 3          # one alive: phat = 1
    assert float(risk[2]) == 2.0                                    # equal scores: the mean of 0, 1, 5, 2
    assert np.all(got[:K, 3] == 0) and float(risk[3]) == 2          # 200 apart: the best row alone counts
    assert got[2, 4] == 0                                           # its error count is not counted
    if has_ref:
        assert got[K].tolist() == [np.float32(ce), np.float32(ce), 0.0, np.float32(ce), np.float32(ce)]
        assert nref.cpu().numpy().tolist() == [4.0, 9.0, 0.0, 55.5, float(nll[4, 4])]


def test_mwer_weights_more_clips_than_one_pass_of_the_workgroup():
    """N = 600 > 256: the clips are walked 256 at a time and the loss is still the index-order fp64 sum"""
    rs = np.random.RandomState(8)
    K, N = 2, 600
    nll = (np.abs(rs.standard_normal((K + 1, N))) * 5 + 1).astype(np.float32)
    err = rs.randint(0, 9, (K, N)).astype(np.int32)
    w, risk, nref, loss = ops.mwer_weights(cu(nll), torch.from_numpy(err).to(DEV), K, True, 0.5)
    rw, rrisk, rnref, rloss, _ = R.weights_rule(nll.astype(np.float64), err, 0.5)
    # where a clip's error counts are equal the exact weight is 0 and both sides hold fp64 rounding residue of err - ebar (a few
    # 2^-53 e_max, depending on the last bit of exp): such values are held to 1e-13 absolute, all others to 1 ulp of fp32
    gw = w.cpu().numpy()
    assert np.all((_ulps(gw, rw.astype(np.float32)) <= 1) | (np.abs(gw - rw) <= 1e-13)), np.abs(gw - rw).max()
    assert _ulps(risk.cpu().numpy(), rrisk.astype(np.float32)).max() <= 1
    assert abs(float(loss.item()) - rloss) <= 1e-6 * abs(rloss)


# ---- MWERLoss end to end ----------------------------------------------------------------------------------------------------
E2E_LENS = [40, 33, 21]


@pytest.fixture(scope="module")
def e2e():
    """N = 3, T' = 40, C = 29, scale 2.0, beam width 8, nbest 4: logits, the decoder's own hypotheses, references.  Random logits
    decode to strings that have nothing in common with a random reference -- every hypothesis would have the same error count --
    so the references are made FROM the list: a lower rank of each clip with a change of its own, which puts the hypotheses at
    different distances (the tests assert that they are)."""
    rs = np.random.RandomState(11)
    Tp, N, Cc, K = 40, 3, 29, 4
    logits = rs.standard_normal((Tp, N, Cc)) * 2.0
    dec = BeamCTCDecoder(LABELS, beam_width=8, blank_index=0)
    out = cu(logits)
    sizes = torch.tensor(E2E_LENS, dtype=torch.int32)
    x = mwer._padded_logits(out)
    probs = ops.softmax_rows(x, Cc).view(Tp, N, Cc).transpose(0, 1)
    toks, lens = dec.nbest_device(probs, sizes.to(DEV), K)
    th, lh = toks.cpu().numpy(), lens.cpu().numpy()
    hyps = [[th[k, n, :lh[k, n]].tolist() if lh[k, n] >= 0 else None for n in range(N)] for k in range(K)]
    assert all(h is not None and len(h) > 4 for row in hyps for h in row)
    refs = [hyps[1][0] + [5, SPACE, 7], list(hyps[1][1]), hyps[2][2][1:]]
    return dict(logits=logits, out=out, sizes=sizes, refs=refs, dec=dec, hyps=hyps, toks=toks, lens=lens, probs=probs,
                targets=torch.tensor(sum(refs, []), dtype=torch.int32), tsz=torch.tensor([len(r) for r in refs], dtype=torch.int32))


def _run(c, unit, ce, nbest=4):
    crit = mwer.MWERLoss(c["dec"], nbest=nbest, ce_weight=ce, unit=unit)
    out = c["out"].clone().requires_grad_(True)
    loss = crit(out, c["targets"], c["sizes"], c["tsz"])
    loss.backward()
    return crit, loss, out.grad


@pytest.mark.parametrize("unit", ["word", "char"])
def test_mwer_loss_end_to_end(e2e, unit):
    c, ce = e2e, 0.05
    Tp, N, Cc = c["logits"].shape
    ref = R.mwer(c["logits"], E2E_LENS, c["hyps"], c["refs"], SPACE, unit, ce)
    # a case whose hypotheses all have the same error count has no risk gradient at all and would show nothing
    assert any(len(set(ref["err"][:, n].tolist())) > 1 for n in range(N)), ref["err"]
    crit, loss, g = _run(c, unit, ce)
    last = crit.last
    assert last["errors"].cpu().numpy().tolist() == ref["err"].tolist()
    assert last["ref_units"].cpu().numpy().tolist() == [R.ref_units(r, SPACE, unit) for r in c["refs"]]
    nll_d = np64(last["nll"])
    fin = np.isfinite(ref["nll"])
    assert np.isfinite(nll_d).tolist() == fin.tolist()
    delta = float(np.abs(nll_d[fin] - ref["nll"][fin]).max())
    assert np.allclose(nll_d[fin], ref["nll"][fin], **NLL_TOL), "delta = %.3e" % delta
    e_max = float(ref["err"].max())
    slack = np.expm1(2 * delta)
    risk_bound = slack * e_max + 1e-6 * e_max
    risk_err = float(np.abs(np64(last["risk"]) - ref["risk"]).max())
    assert risk_err <= risk_bound, "risk error %.3e, bound %.3e (delta %.3e, e_max %g)" % (risk_err, risk_bound, delta, e_max)
    grad_bound = 2 * slack * e_max + (e_max + ce) * grad_bar(Tp)
    grad_err = float(np.abs(np64(g) - ref["dlogits"]).max())
    assert grad_err <= grad_bound, "gradient error %.3e, bound %.3e (delta %.3e, e_max %g)" % (grad_err, grad_bound, delta, e_max)
    print("MWERLoss %s: delta %.3e, risk error %.3e (bound %.3e), gradient error %.3e (bound %.3e)"
          % (unit, delta, risk_err, risk_bound, grad_err, grad_bound))
    assert np.abs(np64(last["posterior"]) - ref["phat"]).max() <= slack + 1e-6
    assert abs(float(loss.item()) - ref["loss"]) <= N * risk_bound + ce * 2e-5 * ref["nll_ref"].sum() + ce * N * 1e-4
    for n in range(N):
        assert torch.all(g[E2E_LENS[n]:, n] == 0)
    want = float(ref["risk"].sum()) / sum(R.ref_units(r, SPACE, unit) for r in c["refs"])
    assert abs(crit.expected_error_rate() - want) <= N * risk_bound
    # a second backward through the same forward: refused, as _CtcFn's
    crit2 = mwer.MWERLoss(c["dec"], nbest=4, ce_weight=ce, unit=unit)
    out = c["out"].clone().requires_grad_(True)
    l2 = crit2(out, c["targets"], c["sizes"], c["tsz"])
    l2.backward(retain_graph=True)
    with pytest.raises(RuntimeError):
        l2.backward()


def test_gradient_step_lowers_the_risk(e2e):
    """hypothesis set held fixed: the reference's risk at logits - eps g / |g| is below the risk at logits, g = the device gradient
    with ce_weight = 0, eps = 1e-2"""
    c = e2e
    _, _, g = _run(c, "word", 0.0)
    g = np64(g)
    assert np.abs(g).max() > 0
    ref = R.mwer(c["logits"], E2E_LENS, c["hyps"], c["refs"], SPACE, "word", 0.0)
    assert any(len(set(ref["err"][:, n].tolist())) > 1 for n in range(3)), ref["err"]
    before = ref["risk"].sum()
    after = R.mwer(c["logits"] - 1e-2 * g / np.sqrt((g ** 2).sum()), E2E_LENS, c["hyps"], c["refs"], SPACE, "word", 0.0)["risk"].sum()
    assert after < before, (after, before)


@pytest.mark.parametrize("N", [2, 3])
def test_nbest_zero_is_plain_ctc_bit_for_bit(e2e, N):
    """MWERLoss(nbest = 0, ce_weight = 1) through CTCLossHip's calling form: the per-clip nll and the gradient have _CtcFn's bits.
    The scalar: _CtcFn adds the clips' nll in fp32 across the lanes of a wave, ds2_mwer_weights in fp64 in index order, rounded once;
    two terms round the same either way (N = 2: bit for bit), for more the scalar is held to the rule itself -- the fp32 rounding of
    the fp64 index-order sum of the very nll bits _CtcFn reports."""
    c = e2e
    out0 = c["out"][:, :N].clone().requires_grad_(True)
    tg, tsz, sizes = c["targets"][:int(c["tsz"][:N].sum())], c["tsz"][:N], c["sizes"][:N]
    l0 = CTCLossHip(blank=0)(out0, tg, sizes, tsz)
    l0.backward()
    crit = mwer.MWERLoss(c["dec"], nbest=0, ce_weight=1.0)
    out1 = c["out"][:, :N].clone().requires_grad_(True)
    l1 = crit(out1, tg, sizes, tsz)
    l1.backward()
    assert torch.equal(out1.grad, out0.grad)
    x = mwer._padded_logits(c["out"][:, :N])
    offs = torch.cumsum(tsz, 0) - tsz
    _, nll, _ = ops.ctc_loss_grad(x, tg.to(DEV), offs.to(DEV, torch.int32), sizes.to(DEV), tsz.to(DEV), 40, N, 29, 0, int(tsz.max()))
    assert torch.equal(crit.last["nll_ref"], nll)
    total = 0.0
    for v in nll.cpu().numpy().astype(np.float64):
        total += v
    assert float(l1.item()) == float(np.float32(total))
    if N == 2:
        assert torch.equal(l1.detach(), l0.detach())
    assert crit.last["errors"].shape == (0, N) and crit.last["ref_units"] is None


def test_ctc_scores_of_the_decoders_own_nbest(e2e):
    """no LM: every exact score is <= the beam's reported -log p (a beam drops non-negative path mass), with the margin of the nll
    bar; and equals ctc_multi_forward's value bit for bit"""
    c = e2e
    Tp, N, Cc = c["logits"].shape
    buf, lens, scores = ops.beam_search_device(c["probs"], c["sizes"].to(DEV), 0, 8, 40, 1.0)
    toks, ln = mwer.rank_major(buf[0], lens, scores[0], 8)
    exact = mwer.ctc_scores(c["out"], c["sizes"], (toks, ln))
    beam = scores[0].t()
    alive = ln >= 0
    assert bool(alive[0].all()) and torch.equal(torch.isinf(exact), ~alive)
    assert bool((exact[alive] <= beam[alive] + (1e-4 + 2e-5 * beam[alive].abs())).all())
    direct, _ = ops.ctc_multi_forward(mwer._padded_logits(c["out"]), toks, ln, c["sizes"].to(DEV), Tp, N, Cc, 0)
    assert torch.equal(exact, direct)
    lists = [[(toks[r, n, :ln[r, n]].tolist() if ln[r, n] >= 0 else None) for n in range(N)] for r in range(8)]
    assert torch.equal(mwer.ctc_scores(c["out"], c["sizes"], lists), exact)
    # the first ranks are what MWERLoss scored
    assert torch.equal(ln[:4], c["lens"])
    for r in range(4):
        for n in range(N):
            assert torch.equal(toks[r, n, :ln[r, n]], c["toks"][r, n, :ln[r, n]])


def test_nbest_device_agrees_with_decode_beams(e2e):
    c = e2e
    strings, _, scores = c["dec"].decode_beams(c["probs"], c["sizes"])
    th, lh = c["toks"].cpu().numpy(), c["lens"].cpu().numpy()
    for n in range(3):
        for k in range(4):
            if np.isinf(float(scores[n, k])):
                assert lh[k, n] == -1
            else:
                assert "".join(LABELS[v] for v in th[k, n, :lh[k, n]]) == strings[n][k]


# ---- model level --------------------------------------------------------------------------------------------------------------
def _model_and_batch():
    torch.manual_seed(0)
    mc = configs.BiDirectionalConfig(rnn_type=configs.RNNType.gru, hidden_size=32, hidden_layers=2)
    m = DeepSpeech(LABELS, mc, 32, configs.AdamConfig(), configs.SpectConfig()).to(DEV).train()
    inputs, targets, pct, tsz = synth.synth_batch(np.array([61, 50]), seed=1)

    def batch():
        return (torch.from_numpy(inputs).to(DEV), torch.from_numpy(targets), torch.from_numpy(pct.copy()), torch.from_numpy(tsz))
    return m, batch


def _step(m, batch):
    m.zero_grad()
    loss = m.training_step(batch(), 0)
    loss.backward()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def test_training_step_with_an_attached_mwer_loss():
    m, batch = _model_and_batch()
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    base_loss, base = _step(m, batch)
    dec = BeamCTCDecoder(LABELS, beam_width=8, blank_index=0)
    # nbest = 0, ce_weight = 1: the default step bit for bit (two clips: see test_nbest_zero_is_plain_ctc_bit_for_bit)
    m.load_state_dict(state)
    m.attach_training_loss(mwer.MWERLoss(dec, nbest=0, ce_weight=1.0))
    loss, grads = _step(m, batch)
    assert torch.equal(loss, base_loss)
    for k in base:
        assert torch.equal(grads[k], base[k]), k
    # the real thing: finite loss, a finite gradient for every parameter
    m.load_state_dict(state)
    crit = mwer.MWERLoss(dec, nbest=4, ce_weight=0.01)
    m.attach_training_loss(crit)
    m.zero_grad()
    loss = m.training_step(batch(), 0)
    loss.backward()
    assert bool(torch.isfinite(loss))
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    assert crit.last["risk"].shape == (2,) and crit.last["posterior"].shape == (4, 2) and crit.expected_error_rate() >= 0
    with pytest.raises(RuntimeError):
        loss.backward()                                           # a second backward raises as _CtcFn's does
    # None restores the default
    m.load_state_dict(state)
    m.attach_training_loss(None)
    loss, grads = _step(m, batch)
    assert torch.equal(loss, base_loss)
    for k in base:
        assert torch.equal(grads[k], base[k]), k
    with pytest.raises(ValueError):
        m.attach_training_loss(object())
