"""The output-layer kernels (ds2_fc_fwd / ds2_fc_bwd, csrc/ds2_fc.hip) against float64 torch on the same bf16-rounded operands.

Bounds (derived, not tuned).  Every product of two bf16 values is exact in fp32, so the only errors are the roundings of the fp32
accumulation: a sum of K terms accumulated in fp32 in ANY order is within K * 2^-23 * sum|a_k b_k| of the exact sum (2^-23 per
addition covers round-to-nearest, 2^-24, and a truncating adder).  Hence, elementwise,
    logits  |err| <= H  * 2^-23 * (|Xh| @ |Wp|^T)
    dW      |err| <= R  * 2^-23 * (|bf16(dl)|^T @ |Xh|)       (the row blocks' partials and their sum are part of the same K = R terms)
    dXh     |err| <= e + 2^-8 * (|ref| + e),  e = Cp * 2^-23 * (|bf16(dl)| @ |Wp|)   (+ half a bf16 ulp, <= 2^-8 relative, of the
                                                                                     rounded result)
Row counts: the kernels work in 32-row tiles (a wave's tile forward, a group of the row block backward), so 31 / 32 / 33 and 2*32+3
are the seams of that block next to the 1 / 255 / 256 / 257 every size set has; 257 rows are 9 groups, one more than the dW kernel's
ring of 8 groups in flight (5 at 64 classes, ring of 4); 8 195 rows give three dW row blocks of 86 groups and dX row blocks of
several groups; 66 000 rows at H = 16 give the forward's waves more than one tile each and dW 32 row blocks."""
import pytest
import torch

from fixtures import Fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
E23 = 2.0 ** -23


def operands(R, H, Cp, C, seed, pad_stride=False):
    """(Xh [R][H] bf16 -- a view with a padded row stride on request --, Wp [Cp][H] bf16 with zero rows >= C, dl [R][Cp] f32 with
    zero columns >= C), seeded on the host."""
    from deepspeech.pytorch_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((R, H), generator=g).to(BF)
    w = (torch.randn((Cp, H), generator=g) * 0.1).to(BF)
    dl = torch.randn((R, Cp), generator=g) * 0.05
    w[C:] = 0
    dl[:, C:] = 0
    if pad_stride:
        ld = ops.pad_ld(H, BF)
        assert ld != H
        X = torch.full((R, ld), float("nan"), dtype=BF, device=DEV)[:, :H]
        X.copy_(x)
    else:
        X = x.to(DEV)
    return X, w.to(DEV), dl.to(DEV)


def reference(X, W, dl):
    """float64 results and the |A| @ |B| sums of the bounds, on the host."""
    x, w = X.detach().cpu().double(), W.detach().cpu().double()
    d = dl.detach().cpu().to(BF).double()
    return dict(logits=x @ w.t(), a_logits=x.abs() @ w.abs().t(), dXh=d @ w, a_dXh=d.abs() @ w.abs(), dW=d.t() @ x,
                a_dW=d.abs().t() @ x.abs())


def bounds(ref, R, H, Cp):
    e = Cp * E23 * ref["a_dXh"]
    return dict(logits=H * E23 * ref["a_logits"], dW=R * E23 * ref["a_dW"], dXh=e + 2.0 ** -8 * (ref["dXh"].abs() + e))


def check(name, got, ref, bound):
    err = (got.detach().cpu().double() - ref[name]).abs()
    worst = float((err - bound[name]).max())
    print("%s: max |err| %.3e, max bound %.3e, max (err - bound) %.3e" % (name, float(err.max()), float(bound[name].max()), worst))
    assert bool((err <= bound[name]).all()), (name, worst)


ROWS = [1, 31, 32, 33, 67, 255, 256, 257]
CASES = [(R, H, Cp, C, False) for R in ROWS for H in (16, 80, 1024) for Cp, C in ((32, 29), (64, 64))]
CASES += [(257, 1024, 32, 29, True), (8195, 1024, 32, 29, False), (8195, 1024, 64, 40, False), (66000, 16, 32, 29, False)]


@pytest.mark.parametrize("R,H,Cp,C,pad", CASES)
def test_fc_entries_against_float64(R, H, Cp, C, pad):
    from deepspeech.pytorch_amd import ops
    assert ops.fc_ok(BF, H, Cp)
    X, W, dl = operands(R, H, Cp, C, seed=R * 131 + H + Cp, pad_stride=pad)
    ref = reference(X, W, dl)
    bound = bounds(ref, R, H, Cp)
    n0 = dict(ops.FC_CALLS)
    logits = ops.fc_fwd(X, W)
    dXh, dW = ops.fc_bwd(dl, X, W)
    assert ops.FC_CALLS["fwd"] == n0["fwd"] + 1 and ops.FC_CALLS["bwd"] == n0["bwd"] + 1
    assert logits.shape == (R, Cp) and dXh.shape == (R, H) and dW.shape == (Cp, H) and dXh.dtype == BF
    check("logits", logits, ref, bound)
    check("dXh", dXh, ref, bound)
    check("dW", dW, ref, bound)
    if C < Cp:      # pad classes: exactly zero
        assert not bool(logits[:, C:].any()) and not bool(dW[C:].any())
    # the summation order is fixed: a second call gives the same bits
    logits2 = ops.fc_fwd(X, W)
    dXh2, dW2 = ops.fc_bwd(dl, X, W)
    assert torch.equal(logits, logits2) and torch.equal(dXh, dXh2) and torch.equal(dW, dW2)


def old_path(X, W, dl):
    """the generic products the head ran before (model._HeadFn without the output-layer kernels)"""
    from deepspeech.pytorch_amd import ops
    R = X.shape[0]
    logits = ops.gemm_nt(X, W, out_dtype=torch.float32)
    d = dl.contiguous().to(BF)
    dXh = ops.gemm_nt(d, W.t().contiguous())
    dW = ops.gemm_nt_kslices(ops.transpose(d), ops.transpose(X), ops.head_kslices(R))
    return logits, dXh, dW


def test_new_path_against_the_generic_products():
    """R = 257, H = 1024: the generic kernels meet the same bounds against float64, and the two paths are within those bounds of
    each other (they are in fact the same bits: the next test)."""
    from deepspeech.pytorch_amd import ops
    R, H, Cp, C = 257, 1024, 32, 29
    X, W, dl = operands(R, H, Cp, C, seed=5)
    ref = reference(X, W, dl)
    bound = bounds(ref, R, H, Cp)
    new = dict(zip(("logits", "dXh", "dW"), (ops.fc_fwd(X, W),) + ops.fc_bwd(dl, X, W)))
    old = dict(zip(("logits", "dXh", "dW"), old_path(X, W, dl)))
    for k in ("logits", "dXh", "dW"):
        check(k, new[k], ref, bound)
        check(k, old[k], ref, bound)
        diff = (new[k].detach().cpu().double() - old[k].detach().cpu().double()).abs()
        print("%s: max |new - old| %.3e" % (k, float(diff.max())))
        assert bool((diff <= bound[k]).all()), k


@pytest.mark.parametrize("R", [257, 8195, 24032])
def test_new_path_keeps_the_bits_of_the_generic_products(R):
    """The kernels keep the generic path's k-steps, their order, the operand slots and -- for dW -- its K-slices (one at R = 257,
    three at 8 195, eight at cfg3's 24 032 rows), so at H = 1024 logits, dXh and dW are the same bits: a training step computes what
    it computed with the generic products."""
    from deepspeech.pytorch_amd import ops
    X, W, dl = operands(R, 1024, 32, 29, seed=R)
    new = (ops.fc_fwd(X, W),) + ops.fc_bwd(dl, X, W)
    old = old_path(X, W, dl)
    for name, a, b in zip(("logits", "dXh", "dW"), new, old):
        print("%s: max |new - old| %.3e" % (name, float((a.double() - b.double()).abs().max())))
        assert torch.equal(a, b), name


def test_model_routes_the_head_through_the_fc_entries(monkeypatch):
    """A small bf16 DeepSpeech: _HeadFn calls both entries once per step, and its gradient of fc.0.module.1.weight is within the
    dW bound of the generic products' result on the very operands the step handed to ds2_fc_bwd."""
    from deepspeech.pytorch_amd import ops
    from test_gpu_model import build
    fx = Fixture("gru_bi_tiny")
    m = build(fx, "bf16").train()
    seen = {}
    real_bwd = ops.fc_bwd

    def spy(dlogits, Xh, Wp, R=None, H=None):
        seen["args"] = (dlogits.clone(), Xh.clone(), Wp.clone())
        return real_bwd(dlogits, Xh, Wp, R, H)

    monkeypatch.setattr(ops, "fc_bwd", spy)
    inputs, targets, pct, tsz = fx.batch()
    batch = (torch.from_numpy(inputs).to(DEV), torch.from_numpy(targets), torch.from_numpy(pct.copy()), torch.from_numpy(tsz))
    n0 = dict(ops.FC_CALLS)
    m.training_step(batch, 0).backward()
    ops.check_persistent_kernels()
    assert ops.FC_CALLS["fwd"] == n0["fwd"] + 1 and ops.FC_CALLS["bwd"] == n0["bwd"] + 1
    dl, Xh, Wp = seen["args"]
    R, H = Xh.shape
    Cp = Wp.shape[0]
    grad = m.fc[0].module[1].weight.grad
    Cc, Ht = grad.shape
    ref = reference(Xh, Wp, dl)
    bound = bounds(ref, R, H, Cp)["dW"][:Cc, :Ht]
    dW_old = old_path(Xh, Wp, dl)[2][:Cc, :Ht].detach().cpu().double()
    got = grad.detach().cpu().double()
    print("fc weight gradient: max |new - old| %.3e, max |new - exact| %.3e, max bound %.3e" % (
        float((got - dW_old).abs().max()), float((got - ref["dW"][:Cc, :Ht]).abs().max()), float(bound.max())))
    assert bool(((got - ref["dW"][:Cc, :Ht]).abs() <= bound).all())
    assert bool(((got - dW_old).abs() <= bound).all())
