"""CPU side of the exact recurrent-sweep tests (tests/rnn_exact_cases.py, tests/test_gpu_rnn_exact.py): the bit budget of the grid in
exact integer / rational arithmetic, agreement of the grid reference with the oracle, and the two SENSITIVITY conditions -- a probe
that cannot see one wrong weight element proves nothing, so the reference alone must notice a swap of two elements of a W_hh row."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

import rnn_exact_cases as X
from oracle import ds2_oracle as O

KINDS = ["gru", "lstm", "rnn"]


def _readouts(op, d, **kw):
    """What the GPU test reads in fp32: hn (and cn) of the length-1 samples."""
    r = X.fwd_first_step(op, d, **kw)
    one = op["lens"] == 1
    return np.concatenate([r["h"][one]] + ([r["c"][one]] if op["kind"] == "lstm" else []), axis=1)


@pytest.mark.parametrize("kind,N,H", [(k, 8, 1024) for k in KINDS] + [("gru", 30, 1536), ("lstm", 64, 1280), ("gru", 3, 32), ("lstm", 20, 48)])
def test_forward_grid_fits_the_fp32_accumulator(kind, N, H):
    """W_hh . h0 + GI + b_hh in integers of 2^-10: the magnitudes of all terms of one pre-activation sum to far less than 2^24, so every
    partial sum in any order is an fp32 number; the float64 product is the integer one; |pre-activation| <= 4, on which the 1e-5 bar of
    the fp32 readout rests (tests/test_gpu_rnn_exact.py)."""
    op = X.fwd_operands(kind, 2, N, H)
    for name, mult in (("Whh", 256), ("h0", 4), ("c0", 4), ("GI", 8), ("bhh", 16)):
        v = op[name] * mult
        assert np.array_equal(v, np.rint(v)), name
        assert torch.equal(X.to_storage(op[name], torch.bfloat16).double(), torch.from_numpy(op[name])), name     # exact in bf16
    assert np.abs(op["Whh"]).max() <= 7 / 256 and np.abs(op["GI"]).max() <= 1 and np.abs(op["bhh"]).max() <= 0.25
    assert set(np.unique(np.abs(op["h0"]))) == {0.25, 0.5, 0.75}
    for d in range(2):
        units, same = X.fwd_budget(op, d)
        assert same and units < 2 ** 24 // 64, units
        assert np.abs(X.fwd_first_step(op, d)["pre"]).max() <= 4.0


@pytest.mark.parametrize("kind", KINDS)
def test_forward_grid_reference_is_the_oracle(kind):
    D, N, H = 2, 6, 32
    G = X.GATES[kind]
    op = X.fwd_operands(kind, D, N, H)
    for d in range(D):
        out, hn, cn, cache = O.rnn_dir_fwd(kind, op["GI"].reshape(X.TP, N, D, G * H)[:, :, d], op["lens"], np.eye(G * H), op["Whh"][d],
                                           np.zeros(G * H), op["bhh"][d], reverse=(d == 1), h0=op["h0"][d], c0=op["c0"][d])
        ref = X.fwd_first_step(op, d)
        one = op["lens"] == 1
        assert np.abs(hn[one] - ref["h"][one]).max() < 1e-15
        assert np.abs(out[ref["t"], np.arange(N)] - ref["h"]).max() < 1e-15
        if kind == "lstm":
            assert np.abs(cn[one] - ref["c"][one]).max() < 1e-15
        st = cache["steps"][0]           # the first processed time index: t = 0 forward, t = 2 reverse (sample 0 only starts there)
        rows = ref["t"] == st["t"]
        if kind == "gru":
            got = np.concatenate([st["r"], st["z"], st["n"], st["hn"]], axis=1)
        elif kind == "lstm":       # the c plane is the state after the step: cn of the samples that end here, checked above
            got = np.concatenate([st["i"], st["f"], st["g"], st["o"], np.arctanh(st["tc"])], axis=1)
        else:
            got, ref["planes"] = st["hnew"], ref["h"]
        assert rows.any() and np.abs(got[rows] - ref["planes"][rows]).max() < 1e-14


@pytest.mark.parametrize("kind", KINDS)
def test_forward_swaps_of_two_weights_move_an_fp32_readout(kind):
    """300 random swaps of two elements of one W_hh row: at least 90 % move hn / cn of a length-1 sample by more than 1e-4, ten times
    the GPU test's bar (the rest exchange equal weights, or weights on equal states, and change nothing)."""
    D, N, H = 1, 8, 1024
    op = X.fwd_operands(kind, D, N, H)
    base = _readouts(op, 0)
    rs = np.random.RandomState(5)
    seen, smallest = 0, np.inf
    for _ in range(300):
        row, k1, k2 = rs.randint(X.GATES[kind] * H), *rs.choice(H, 2, replace=False)
        move = np.abs(_readouts(op, 0, Whh=X.swap_in_row(op["Whh"][0], row, k1, k2)) - base).max()
        seen += move > 1e-4
        if move > 0:
            smallest = min(smallest, move)
    print("forward swaps seen: %s %d of 300, smallest non-zero effect %.2e" % (kind, seen, smallest))
    assert seen >= 270, seen


@pytest.mark.parametrize("kind", KINDS)
def test_forward_dropped_k_chunk_and_shifted_sample_are_seen(kind):
    op = X.fwd_operands(kind, 1, 8, 1024)
    base = _readouts(op, 0)
    W = op["Whh"][0].copy()
    W[:, 32:64] = 0                                              # one 32-element k-step left out
    assert np.abs(_readouts(op, 0, Whh=W) - base).max() > 100 * 1e-5
    assert np.abs(_readouts(op, 0, h0=np.roll(op["h0"][0], 1, axis=0)) - base).max() > 100 * 1e-5       # rows of the state shifted by one


# ---- BPTT -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_bptt_grid_reference_is_the_oracle(kind, state):
    D, N, H = 2, 5, 32
    G = X.GATES[kind]
    op = X.bwd_operands(kind, D, N, H, state=state)
    two = op["lens"] == 2
    for d in range(D):
        dx, _, _, _, _, dh0, dc0 = O.rnn_dir_bwd(X.oracle_cache(op, d), op["dOut"], np.eye(G * H), op["Whh"][d], return_dstate=True)
        first = X.bwd_first_step(op, d)
        sec = X.bwd_second_step(op, d, first, first["dgh"])
        ar = np.arange(N)
        assert np.abs(dx[first["t"], ar] - first["dgi"]).max() < 1e-15
        assert np.abs(dx[sec["t"], ar] - sec["dgi"])[sec["rows"]].max() < 1e-14
        assert np.abs(dh0 - (sec["ch"] + sec["dgh"] @ op["Whh"][d]))[two].max() < 1e-14
        if kind == "lstm":
            assert np.abs(dc0 - sec["cc"])[two].max() < 1e-14
        one = op["lens"] == 1
        assert one.any() == state
        if state:                       # a length-1 sample's first processed step is its last
            assert np.abs(dh0 - (first["ch"] + first["dgh"] @ op["Whh"][d]))[one].max() < 1e-14
            if kind == "lstm":
                assert np.abs(dc0 - first["cc"])[one].max() < 1e-14


def _frac_second_step(op, d, first, dgh1, sec, n, j):
    """Output (n, j) of the second processed step in exact rational arithmetic: the gate-gradient slots of dGI and the hidden-side n slot."""
    kind, H = op["kind"], op["H"]
    F = lambda v: Fraction(float(v))
    W = op["Whh"][d]
    t = int(sec["t"][n])
    dh = F(op["dOut"][t, n, j]) + F(first["ch"][n, j]) + sum(F(a) * F(w) for a, w in zip(dgh1[n], W[:, j]) if a != 0 and w != 0)
    P, hprev, cprev, hcur = X._step_inputs(op, d, sec["t"])
    if kind == "gru":
        r, z, nn, q = (F(P[n, k * H + j]) for k in range(4))
        dn = dh * (1 - z) * (1 - nn * nn)
        return [dn * q * r * (1 - r), dh * (F(hprev[n, j]) - nn) * z * (1 - z), dn, dn * r]
    if kind == "lstm":
        i, f, g, o, c = (F(P[n, k * H + j]) for k in range(5))
        assert c == 0                                    # tanh(0) = 0 exactly: the formulas are polynomials here
        dcn = F(first["cc"][n, j]) + dh * o
        return [dcn * g * i * (1 - i), dcn * F(cprev[n, j]) * f * (1 - f), dcn * i * (1 - g * g), Fraction(0)]
    return [dh * (1 - F(hcur[n, j]) ** 2)]


PROOF_CASES = sorted({(dt, kind, N, H) for dt, kind, D, N, H, v, f in X.ALL_CASES})


@pytest.mark.parametrize("dt,kind,N,H", PROOF_CASES, ids=lambda v: str(v))
def test_bptt_second_step_is_exact_per_case(dt, kind, N, H):
    """For every (storage, cell, N, H) the GPU test runs: with the first step's gradients rounded to the storage type (what a correct
    device stores and its product consumes), every term of dh = dOut + carry + dgates . W_hh is an integer number of 2^-(q + 8) and
    their magnitudes sum to less than 2^24 units (exact_rows), each compared output has at most 24 significant bits, and float64 gives
    the same value as rational arithmetic.  The one exception is stated, not hidden: fp32 storage keeps tanh(c) of the LSTM's first step
    in 24 bits; there only sample 0 has c != 0 at that step, its sum is not exact, and every other sample's is."""
    dtype = getattr(torch, dt)
    f32_lstm = kind == "lstm" and dtype == torch.float32
    op = X.bwd_operands(kind, 1, N, H, fp32=dtype == torch.float32)
    G = X.GATES[kind]
    first = X.bwd_first_step(op, 0)
    if kind != "lstm":
        assert X.fits24(first["dgi"]).all() and X.fits24(first["dgh"]).all()         # the first step is stored correctly rounded
    else:
        units = X.compared_units(op)
        with_tanh = np.arange(N) < 1 if f32_lstm else np.ones(N, dtype=bool)
        assert (first["dgi"][:, 3 * H:][~units & with_tanh[:, None]] != 0).all()       # do carries data
        assert (first["dgi"][:, H:2 * H][~units] != 0).all()                           # df carries data
        assert (first["dgi"][:, :H] != 0).all() and (first["dgi"][:, 2 * H:3 * H] != 0).all()
    dgh1 = X.as64(X.to_storage(first["dgh"], dtype)) if dtype == torch.bfloat16 else first["dgh"].astype(np.float32).astype(np.float64)
    sec = X.bwd_second_step(op, 0, first, dgh1)
    units = X.compared_units(op)
    if f32_lstm:
        assert not sec["exact"][0] and sec["exact"][1:].all()
        assert X.fits24(first["dgh"][1:]).all()
        units = units & (np.arange(N) > 0)[:, None]
    else:
        assert sec["exact"].all()
    cand = np.argwhere(units)
    assert X.fits24(sec["dh"][units]).all()
    units = np.tile(units, (1, G))
    assert X.fits24(sec["dgi"][units]).all() and X.fits24(sec["dgh"][units]).all()
    assert (np.abs(sec["dgi"]).sum(0) > 0).all()
    rs = np.random.RandomState(N + H)
    for n, j in cand[rs.choice(len(cand), 12, replace=False)]:
        exact = _frac_second_step(op, 0, first, dgh1, sec, n, j)
        got = [sec["dgi"][n, g * H + j] for g in range(G)] + ([sec["dgh"][n, 2 * H + j]] if kind == "gru" else [])
        assert [Fraction(float(v)) for v in got] == exact, (n, j)
        assert all(abs(e.numerator) < 2 ** 24 for e in exact)


def test_bptt_swaps_of_two_weights_change_a_stored_gradient():
    """Of 300 random swaps of two elements of a W_hh row, at least 95 % of those that change the product at all change a bf16 dGI that
    the GPU test compares bit for bit."""
    kind, N, H = "gru", 8, 1024
    op = X.bwd_operands(kind, 1, N, H)
    first = X.bwd_first_step(op, 0)
    dgh1 = X.as64(X.to_storage(first["dgh"], torch.bfloat16))
    base = X.bwd_second_step(op, 0, first, dgh1)
    stored = X.to_storage(base["dgi"], torch.bfloat16)
    rs = np.random.RandomState(6)
    changed = seen = 0
    for _ in range(300):
        row, k1, k2 = rs.randint(X.GATES[kind] * H), *rs.choice(H, 2, replace=False)
        W = X.swap_in_row(op["Whh"][0], row, k1, k2)
        delta = dgh1[:, row] * (W[row, k1] - op["Whh"][0][row, k1])          # what the swap adds to dh[:, k1] (and takes from dh[:, k2])
        if not delta.any():
            continue
        changed += 1
        dh = base["dh"].copy()
        dh[:, k1] += delta
        dh[:, k2] -= delta
        P, hprev, cprev, hcur = X._step_inputs(op, 0, base["t"])
        dgi = X.gate_grads(kind, H, dh, np.zeros_like(dh), P, hprev, cprev, hcur)[0]
        seen += not torch.equal(X.to_storage(dgi, torch.bfloat16), stored)
    print("BPTT swaps: %d of %d that change the product change a stored bf16 dGI" % (seen, changed))
    assert changed >= 250 and seen >= 0.95 * changed, (seen, changed)


def _swaps(rs, G, H, count=300):
    for _ in range(count):
        yield (rs.randint(G * H), *rs.choice(H, 2, replace=False))


def test_bptt_swaps_change_an_fp32_lstm_gradient_that_is_compared_exactly():
    """fp32 storage, LSTM (launch-per-step and family 4): of the swaps that change the recurrent product of a sample whose second step
    is compared bit for bit (every sample but 0), at least 95 % change an fp32 dGI at a compared unit.  Swaps in the o rows change
    nothing for these samples (do = 0): the o slot of fp32 LSTM is seen by sample 0's coarse bound only."""
    kind, N, H = "lstm", 8, 1024
    op = X.bwd_operands(kind, 1, N, H, fp32=True)
    first = X.bwd_first_step(op, 0)
    dgh1 = first["dgh"].astype(np.float32).astype(np.float64)
    base = X.bwd_second_step(op, 0, first, dgh1)
    rows = base["exact"]
    assert rows[1:].all() and not rows[0]
    units = np.tile(X.compared_units(op) & rows[:, None], (1, 4))
    P, hprev, cprev, hcur = X._step_inputs(op, 0, base["t"])
    changed = seen = 0
    for row, k1, k2 in _swaps(np.random.RandomState(8), 4, H):
        delta = dgh1[:, row] * (op["Whh"][0][row, k2] - op["Whh"][0][row, k1]) * rows
        if not delta.any():
            continue
        changed += 1
        dh = base["dh"].copy()
        dh[:, k1] += delta
        dh[:, k2] -= delta
        dgi = X.gate_grads(kind, H, dh, base["dc"], P, hprev, cprev, hcur)[0]
        seen += bool((dgi.astype(np.float32) != base["dgi"].astype(np.float32))[units].any())
    print("fp32 LSTM BPTT swaps: %d of %d seen" % (seen, changed))
    assert changed >= 180 and seen >= 0.95 * changed, (seen, changed)


@pytest.mark.parametrize("kind", KINDS)
def test_bptt_swaps_change_dh0_of_a_length_1_sample(kind):
    """dh0 of the launch-per-step BPTT, bf16 storage: of the swaps that change the folded product of a length-1 sample, at least 95 %
    change its fp32 dh0 (compared bit for bit)."""
    N, H = 9, 1024
    G = X.GATES[kind]
    op = X.bwd_operands(kind, 1, N, H, state=True)
    one = op["lens"] == 1
    first = X.bwd_first_step(op, 0)
    D1 = X.as64(X.to_storage(first["dgh"], torch.bfloat16))
    W = op["Whh"][0]
    assert one.sum() == 3 and X.exact_rows(D1, np.abs(first["ch"]) + np.abs(D1) @ np.abs(W))[one].all()
    base = (first["ch"] + D1 @ W)[one]
    assert X.fits24(base).all()
    changed = seen = 0
    for row, k1, k2 in _swaps(np.random.RandomState(9), G, H):
        delta = D1[one, row] * (W[row, k2] - W[row, k1])
        if not delta.any():
            continue
        changed += 1
        got = base.copy()
        got[:, k1] += delta
        got[:, k2] -= delta
        seen += bool((got.astype(np.float32) != base.astype(np.float32)).any())
    print("dh0 swaps: %s %d of %d seen" % (kind, seen, changed))
    assert changed >= 200 and seen >= 0.95 * changed, (seen, changed)


def test_the_cases_reach_the_families_they_claim():
    """The routing of every persistent case on a full device (ds2_rnn_persist_plan with 256 compute units: arithmetic only)."""
    from deepspeech.pytorch_amd import _lib
    lib = _lib.load()
    cells = {"gru": _lib.CELL_GRU, "lstm": _lib.CELL_LSTM, "rnn": _lib.CELL_RNN_TANH}
    for dt, kind, D, N, H, variant, family in X.ALL_CASES:
        if family:
            got = lib.ds2_rnn_persist_plan(_lib.F32 if dt == X.F32 else _lib.BF16, cells[kind], D, N, H, 256, variant, C.POINTER(C.c_long)())
            assert got == family, (dt, kind, D, N, H, variant, got)
    assert {c[6] for c in X.ALL_CASES} == {0, 1, 2, 3, 4}
    assert {c[4] for c in X.FAMILY3_CASES} == {384, 512, 640, 768, 800, 896, 1024, 1152, 1280, 1408, 1536}
