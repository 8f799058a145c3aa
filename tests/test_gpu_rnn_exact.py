"""The recurrent sweeps on exact dyadic operands (tests/rnn_exact_cases.py), every kernel family: the launch-per-step kernels
(csrc/ds2_rnn.hip), the tuned H = 1024 kernels (ds2_rnn_persist_impl.h, families 1 and 2), the round-2 general kernels
(ds2_rnn_persist2_impl.h, family 4) and the round-4 general kernels (ds2_rnn_persist3_impl.h, family 3).

On the grid every partial sum of the recurrent product is exact in fp32 in any order, so one W_hh element paired with the wrong
h[k] -- a wrong lane-to-slot map, LDS-tail offset or compressed-A slot -- moves a compared value by far more than the bars here:
  forward   fp32 readout hn / cn of the length-1 samples within 1e-5 of float64 (only the gate functions differ: v_exp_f32 and
            v_rcp_f32 at 1 ulp give <= 2e-7 per sigmoid, 4e-7 per tanh, about 2e-6 through the cell update; the bar is five times
            that); stored h_t and planes of every sample's first step the rounded reference or its neighbour (near zero, where a
            bf16 ulp is finer than the gate functions: the rounding of a value within 1e-5); the GRU's W_hn h + b_hn plane bit for bit.
  BPTT      first processed step: stored gate gradients within one storage ulp (GRU, RNN: exactly the reference); second processed
            step: dGI (and dQ / dGH) bit for bit the correctly rounded exact value formed from the device's own first-step gradients;
            bacc of the length-2 samples bit for bit the sum of the stored planes.
            dh0 / dc0 of the launch-per-step BPTT: bit for bit for the length-1 samples (lengths a third each of 3, 2, 1 there).
Two comparisons cannot be exact and are coarse guards only, K * 2^-24 * sum |terms| (about 1e-3 at H = 1024: they see a dropped
k-chunk, not one weight; tests/rnn_exact_cases.py says why): sample 0 of the fp32-storage LSTM cases, the one sample there whose first
step keeps tanh(c), and dh0 of the length-2 samples.
Each case: one forward and one BPTT launch (the launch-per-step kernels: a second BPTT with h0 / c0 and want_dstate)."""
import numpy as np
import pytest
import torch

import rnn_exact_cases as X
from fixtures import DEV

pytestmark = pytest.mark.gpu

READOUT_BAR = 1e-5


def ops():
    from deepspeech.pytorch_amd import ops as _ops
    return _ops


class _route:
    """The routing of one case: the launch-per-step kernels (family 0) or a persistent family under its routing bits."""

    def __init__(self, o, variant, family):
        self.o, self.variant, self.family = o, variant, family

    def __enter__(self):
        self.old = self.o.PERSIST_ENABLED
        self.o.PERSIST_ENABLED = self.family != 0
        self.opts = self.o.persist_options(variant=self.variant)
        self.opts.__enter__()

    def __exit__(self, *exc):
        self.opts.__exit__(*exc)
        self.o.PERSIST_ENABLED = self.old
        return False


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype).contiguous()


def _rows(x, t, N):
    """x [T'][N][...] CPU tensor -> [N][...]: row t[n] of sample n."""
    return x[torch.from_numpy(t), torch.arange(N)]


def _launched(o, case):
    dt, kind, D, N, H, variant, family = case
    dtype = getattr(torch, dt)
    if family:
        assert o.persist_kind(dtype, kind, D, N, H) == family, "the case does not reach the family it claims"
        assert o.use_persistent(kind, dtype, D, N, H)
    return dtype


def run_forward(case, swap=None):
    """One forward launch on grid operands and every check of the first processed step.  swap = (d, row, k1, k2): exchange two
    elements of the DEVICE's W_hh only."""
    o = ops()
    dt, kind, D, N, H, variant, family = case
    G, NS = X.GATES[kind], X.PLANES[kind]
    op = X.fwd_operands(kind, D, N, H)
    Wdev = op["Whh"]
    if swap is not None:
        Wdev = X.swap_in_row(op["Whh"], (swap[0], swap[1]), swap[2], swap[3])
        assert not np.array_equal(Wdev, op["Whh"])
    with _route(o, variant, family):
        dtype = _launched(o, case)
        lens_d = torch.from_numpy(op["lens"].astype(np.int32)).to(DEV)
        hext, Sv, hn, cn = o.rnn_fwd(kind, _dev(op["GI"], dtype), _dev(Wdev, dtype), _dev(op["bhh"]), lens_d, D, N, H, X.TP,
                                     h0=_dev(op["h0"]), c0=_dev(op["c0"]) if kind == "lstm" else None)
        if family:
            o.check_persistent_kernels()
    hext, hn = hext.cpu(), X.as64(hn)
    Sv = Sv.cpu() if NS else None
    cn = X.as64(cn) if kind == "lstm" else None
    one = op["lens"] == 1
    worst = 0.0
    for d in range(D):
        ref = X.fwd_first_step(op, d)
        assert np.abs(ref["pre"]).max() <= 4.0
        # fp32 readout of the length-1 samples: their first step is their last
        err = np.abs(hn[d][one] - ref["h"][one]).max()
        if kind == "lstm":
            err = max(err, np.abs(cn[d][one] - ref["c"][one]).max())
        worst = max(worst, err)
        print("rnn-exact readout: family %d %s d=%d max |hn - float64| = %.3e (bar %.0e)" % (family, X.case_id(case), d, err, READOUT_BAR))
        assert err <= READOUT_BAR, (X.case_id(case), d, "readout", err)
        # stored h_t and planes of every sample's first processed step
        msg = X.near_stored(_rows(hext[d, 1:X.TP + 1], ref["t"], N), ref["h"], dtype)
        assert not msg, (X.case_id(case), d, "hext", msg)
        if NS:
            got = _rows(Sv[d], ref["t"], N)
            msg = X.near_stored(got, ref["planes"], dtype)
            assert not msg, (X.case_id(case), d, "saved planes", msg)
            if kind == "gru":       # W_hn h + b_hn: no gate function, the correctly rounded exact value
                q = ref["planes"][:, 3 * H:]
                assert X.fits24(q).all()
                assert torch.equal(got[:, 3 * H:], X.to_storage(q, dtype)), (X.case_id(case), d, "hn plane")
    return worst


def _second_step_check(case, op, d, dtype, dev_gi, dev_gh, sec, what):
    """dev_gi / dev_gh [N, G*H] CPU tensors (storage type) of the second processed step against `sec` (X.bwd_second_step)."""
    kind, N, H = op["kind"], op["N"], op["H"]
    G = X.GATES[kind]
    units = np.tile(X.compared_units(op) & sec["rows"][:, None], (1, G))
    exact = sec["exact"]
    proven = sec["rows"].copy()          # samples whose sum must be provably exact: all with a second step ...
    if kind == "lstm" and dtype == torch.float32:
        proven[0] = False                # ... but fp32 LSTM's sample 0, which keeps tanh(c) in its first step (coarse bound below)
    assert exact[proven].all(), (X.case_id(case), d, what, "the recurrent sum leaves the 24-bit budget")
    K = G * H + 2
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -23
    for name, dev, ref, gain in (("dGI", dev_gi, sec["dgi"], sec["gain_gi"]), ("dGH", dev_gh, sec["dgh"], sec["gain_gh"])):
        m_exact = units & exact[:, None]
        assert X.fits24(ref[m_exact]).all(), (X.case_id(case), d, what, name)
        same = (dev == X.to_storage(ref, dtype)).numpy()
        assert same[m_exact].all(), (X.case_id(case), d, what, name, "wrong elements (n, k): %s" % np.argwhere(m_exact & ~same)[:8].tolist())
        m_bound = units & ~exact[:, None]
        tol = X.fp32_sum_bound(np.tile(sec["absum"], (1, G)), K) * gain + eps * np.abs(ref)
        assert (np.abs(X.as64(dev) - ref) <= tol)[m_bound].all(), (X.case_id(case), d, what, name)


def run_bptt(case, state=False):
    """One BPTT launch on fabricated grid planes: first processed step, second processed step, bacc (persistent), dh0 / dc0 (state)."""
    o = ops()
    dt, kind, D, N, H, variant, family = case
    G, NS = X.GATES[kind], X.PLANES[kind]
    op = X.bwd_operands(kind, D, N, H, state=state, fp32=dt == X.F32)
    ar = torch.arange(N)
    with _route(o, variant, family):
        dtype = _launched(o, case)
        lens_d = torch.from_numpy(op["lens"].astype(np.int32)).to(DEV)
        Sv = _dev(op["Sv"], dtype) if NS else torch.empty(1, dtype=dtype, device=DEV)
        kw = {}
        if state:
            kw = dict(h0=_dev(op["h0"]), c0=_dev(op["c0"]) if kind == "lstm" else None, want_dstate=True)
        rg = o.rnn_bwd(kind, _dev(op["dOut"], dtype), _dev(op["Whh"].transpose(0, 2, 1), dtype), _dev(op["hext"], dtype), Sv, lens_d,
                       D, N, H, X.TP, **kw)
        if family:
            o.check_persistent_kernels()
    dgi = rg.dGI.cpu().reshape(X.TP, N, D, G * H)
    assert (rg.bacc is not None) == (family != 0) and (rg.dGH is not None) == (family == 0 and kind == "gru")
    one, two = op["lens"] == 1, op["lens"] == 2
    for d in range(D):
        def hidden_side(t):
            """[N, G*H] what the device stored for d(W_hh h + b_hh) at each sample's step t[n], and its dGI rows."""
            gi = dgi[torch.from_numpy(t), ar, d]
            if kind != "gru":
                return gi, gi
            if rg.dGH is not None:
                gh = _rows(rg.dGH[d].cpu(), t, N)
                assert torch.equal(gh[:, :2 * H], gi[:, :2 * H])
                return gi, gh
            return gi, torch.cat([gi[:, :2 * H], _rows(rg.dQ[d].cpu(), t, N)], dim=1)

        first = X.bwd_first_step(op, d)
        gi1, gh1 = hidden_side(first["t"])
        for name, dev, ref in (("dGI", gi1, first["dgi"]), ("dGH", gh1, first["dgh"])):
            if kind == "lstm":
                msg = X.near_stored(dev, ref, dtype)
                assert not msg, (X.case_id(case), d, "first step", name, msg)
            else:
                assert X.fits24(ref).all()
                assert torch.equal(dev, X.to_storage(ref, dtype)), (X.case_id(case), d, "first step", name)
        # second processed step: from the gradients the device stored at the first
        sec = X.bwd_second_step(op, d, first, X.as64(gh1))
        gi2, gh2 = hidden_side(sec["t"])
        _second_step_check(case, op, d, dtype, gi2, gh2, sec, "second step")
        if rg.bacc is not None:      # length-2 samples: both steps in hand; two fp32 terms add the same way in either order
            NB = 4 if kind == "gru" else G
            tot = X.as64(dgi[:, :, d]).sum(0)
            if kind == "gru":
                tot = np.concatenate([tot, X.as64(rg.dQ[d].cpu()).sum(0)], axis=1)
            got = rg.bacc[d].cpu()
            assert got.shape == (N, NB * H)
            assert torch.equal(got[two], X.to_storage(tot, torch.float32)[two]), (X.case_id(case), d, "bacc")
        if state:
            # length-1 samples: the first processed step is the last, dh0 = carry + (its stored gradients) . W_hh is an exact readout
            W = op["Whh"][d]
            D1 = X.as64(gh1)
            ref1 = first["ch"] + D1 @ W
            assert one.any() and X.exact_rows(D1, np.abs(first["ch"]) + np.abs(D1) @ np.abs(W))[one].all(), (X.case_id(case), d, "dh0 budget")
            assert X.fits24(ref1[one]).all()
            assert np.array_equal(X.as64(rg.dh0[d])[one], ref1[one]), (X.case_id(case), d, "dh0 of the length-1 samples")
            if kind == "lstm":           # dc0 = dcn * f: exact where tanh(c) = 0
                m1 = one[:, None] & (np.ones_like(op["cmask"]) if dtype == torch.float32 else op["cmask"])
                assert m1.any() and np.array_equal(X.as64(rg.dc0[d])[m1], first["cc"][m1]), (X.case_id(case), d, "dc0 of the length-1 samples")
            # length-2 samples fold the SECOND step's stored gradients: not exact (units down to 2^-31), a coarse guard only
            D2 = X.as64(gh2)
            ref0 = sec["ch"] + D2 @ W
            absum = np.abs(sec["ch"]) + np.abs(D2) @ np.abs(W)
            ex = X.exact_rows(D2, absum)
            got = X.as64(rg.dh0[d])
            tol = np.where(ex[:, None], 0.0, X.fp32_sum_bound(absum, G * H + 1))
            print("rnn-exact dh0: %s d=%d rows proven exact %d of %d, max |dh0 - exact| = %.3e" %
                  (X.case_id(case), d, int(ex[two].sum()), int(two.sum()), np.abs(got - ref0)[two].max()))
            assert (np.abs(got - ref0) <= tol)[two].all(), (X.case_id(case), d, "dh0")
            if kind == "lstm":
                m = two[:, None] & X.compared_units(op)
                tolc = np.where(sec["exact"][:, None], 0.0, X.fp32_sum_bound(sec["absum"], G * H + 2) * sec["gain_cc"] + 2.0 ** -23 * np.abs(sec["cc"]))
                assert (np.abs(X.as64(rg.dc0[d]) - sec["cc"]) <= tolc)[m].all(), (X.case_id(case), d, "dc0")


def run_case(case):
    run_forward(case)
    run_bptt(case)
    if case[6] == 0:
        run_bptt(case, state=True)


def swapped_weight_is_caught(case):
    """A deliberate exchange of two W_hh elements in the device operand (not in the reference's copy) must fail the case."""
    dt, kind, D, N, H, variant, family = case
    op = X.fwd_operands(kind, D, N, H)
    d, row, n = D - 1, (X.GATES[kind] - 1) * H + H // 2 + 1, 2          # a length-1 sample reads it out in fp32
    k1, k2 = X.loudest_swap(op, d, row, n)
    with pytest.raises(AssertionError, match="readout|hext|saved planes|hn plane"):      # a comparison failed, not the routing asserts
        run_forward(case, swap=(d, row, k1, k2))


@pytest.mark.parametrize("case", X.PER_STEP_CASES, ids=X.case_id)
def test_launch_per_step_sweeps_on_exact_operands(case):
    run_case(case)


@pytest.mark.parametrize("case", X.TUNED_CASES, ids=X.case_id)
def test_tuned_persistent_sweeps_on_exact_operands(case):
    run_case(case)


@pytest.mark.parametrize("case", X.FAMILY4_CASES, ids=X.case_id)
def test_general_persistent_sweeps_on_exact_operands(case):
    run_case(case)


@pytest.mark.parametrize("case", X.FAMILY3_CASES, ids=X.case_id)
def test_persist3_sweeps_on_exact_operands(case):
    run_case(case)


@pytest.mark.parametrize("case", [X.PER_STEP_CASES[3], X.TUNED_CASES[0], X.TUNED_CASES[8], X.FAMILY4_CASES[6], X.FAMILY3_CASES[13]],
                         ids=X.case_id)
def test_a_swapped_weight_in_the_device_operand_fails_the_case(case):
    swapped_weight_is_caught(case)
