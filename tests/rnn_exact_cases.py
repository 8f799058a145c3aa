"""Operands on a dyadic grid for the recurrent sweeps, and their float64 reference (tests/test_rnn_exact_host.py proves the bit budget
and the sensitivity on the CPU, tests/test_gpu_rnn_exact.py runs the kernels).

Why a grid: with W_hh = k/256 (|k| <= 7) and a state in multiples of 1/4 every term of the recurrent product is an integer number of
2^-10, and so is every partial sum in ANY order -- the fp32 accumulators of the kernels (MFMA chains, K split over waves, LDS
reductions) hold them exactly as long as the sum of the terms' magnitudes stays below 2^24 units.  The product then has one right
answer and a single wrong (row, k) pairing shows.

Forward: T' = 3, lengths [3, 2, 1, 1, ...]; every sample's FIRST processed step (t = 0 forward, t = len - 1 reverse) starts from a
given h0 / c0, so its pre-activation is exact and only the gate functions separate the device from float64.
BPTT: T' = 3, lengths half 3, half 2; hext and the saved planes are fabricated on the grid (rnn_bwd takes them as inputs).  The first
processed step (t = len - 1 forward, t = 0 reverse) has no recurrent term; the SECOND one consumes the first step's stored gate
gradients through W_hh^T.  The reference of the second step is formed from the gradients the DEVICE stored at the first step (they
are what its product consumed), exactly; unit_exp / exact_rows say per sample whether every partial sum fits 24 bits.

LSTM: tanh(c) is the one non-polynomial of BPTT.  Units with (j + n) % 3 == 0 ("cmask") have c = 0 at their first two processed
steps: tanh is exactly 0 there, their cell-state carry is dyadic, and their second-step outputs are compared bit for bit.  The other
units have c != 0 everywhere: they make do and df non-zero, so all 4H slots of the contraction carry data into the compared units.
The mask moves with n, so with three or more samples every output column is compared bit for bit for some sample, and every
contraction slot (g, j') is fed by some sample.
fp32 storage keeps tanh(c) in 24 bits, and a first-step gradient that carries it makes no exact product.  There every sample but
sample 0 has c = 0 at ALL units of its first processed step: its gradients are dyadic and its second step is compared bit for bit
(do = 0: the o slot of W_hh^T carries no data for these samples; df is fed by c_prev != 0 as before).  Sample 0 keeps c != 0: its
sum runs through all 4H slots and is held to the any-order fp32 bound K * 2^-24 * sum |terms| only -- about 1e-3 at H = 1024, a
guard against a dropped k-chunk in the o slot, NOT a probe for one weight (stated, not hidden: tests/test_rnn_exact_host.py holds
the sensitivity condition for the exact samples).

dh0 / dc0 of the launch-per-step BPTT (state = True): lengths a third 3, a third 2, a third 1.  A length-1 sample's first processed
step is its last, so its dh0 = carry + (first-step gradients) . W_hh is an exact fp32 readout, compared bit for bit.  A length-2
sample folds SECOND-step gradients, whose units reach 2^-31: not exact in any design that keeps T' = 3, held to the same coarse bound.
"""
import numpy as np
import torch

GATES = {"gru": 3, "lstm": 4, "rnn": 1}
PLANES = {"gru": 4, "lstm": 5, "rnn": 0}
TP = 3
STATE_GRID = np.array([-0.75, -0.5, -0.25, 0.25, 0.5, 0.75])


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def weights(rs, D, G, H):
    return rs.randint(-7, 8, (D, G * H, H)) / 256.0


# ---- storage helpers ---------------------------------------------------------------------------------------------------------------
def to_storage(a, dtype):
    """float64 numpy -> CPU tensor of the storage type (round to nearest even; the values compared bit for bit fit fp32, so the
    float64 -> float32 -> bf16 route rounds once)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.float32).to(dtype)


def as64(t):
    return t.detach().to("cpu").to(torch.float64).numpy()


def fits24(x):
    """True where the float64 value has at most 24 significant bits (is an fp32 number)."""
    return x.astype(np.float32).astype(np.float64) == x


def bf16_line(x):
    """The bit patterns of a CPU bf16 tensor laid on one line (sign-magnitude -> ordered integers)."""
    i = x.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def bf16_ulps(a, b):
    """Distance of two CPU bf16 tensors in representable values."""
    return (bf16_line(a) - bf16_line(b)).abs()


def near_stored(dev, ref64, dtype):
    """dev (CPU tensor, storage type) is the reference rounded to the storage type or its neighbour: one ulp in bf16, 1e-5 in fp32.
    Near zero a bf16 ulp is finer than the fp32 value's own bar (|h| = 3e-5 has ulps of 2.4e-7, the gate functions are good to
    2e-6): there the stored value must be the rounding of SOME value within 1e-5 of the reference.  Returns "" or what is wrong."""
    if dtype == torch.bfloat16:
        line = bf16_line
        u = bf16_ulps(dev, to_storage(ref64, dtype))
        inside = (line(dev) >= line(to_storage(ref64 - 1e-5, dtype))) & (line(dev) <= line(to_storage(ref64 + 1e-5, dtype)))
        bad = (u > 1) & ~inside
        if bool(bad.any()):
            k = int(torch.argmax(u * bad))
            return "%d elements off; worst %d ulps: stored %r, reference %r" % (int(bad.sum()), int(u.reshape(-1)[k]),
                                                                                 float(dev.reshape(-1)[k]), float(ref64.reshape(-1)[k]))
        return ""
    err = np.abs(as64(dev) - ref64)
    return "" if err.max() <= 1e-5 else "max error %.3e at %s" % (err.max(), np.unravel_index(int(err.argmax()), err.shape))


def unit_exp(x, qmax=80):
    """Per row of x [N, K]: the smallest q with x * 2^q integer for the whole row (values are dyadic; qmax ends non-dyadic input)."""
    y = np.array(x, dtype=np.float64)
    q = np.zeros(y.shape[0], dtype=np.int64)
    for _ in range(qmax):
        bad = np.any(y != np.rint(y), axis=1)
        if not bad.any():
            break
        q[bad] += 1
        y[bad] *= 2.0
    return q


def exact_rows(dgh, absum):
    """Rows (samples) whose recurrent sum is exact in fp32 in any order: every term dgh[n, k] * W[k, j] is an integer number of
    2^-(q_n + 8); the magnitudes of all terms of one output (absum, with dOut and the carry) stay below 2^24 of them."""
    q = unit_exp(dgh)
    return absum.max(axis=1) * np.exp2(q + 8.0) < 2.0 ** 24


# ---- forward -------------------------------------------------------------------------------------------------------------------------
def fwd_lens(N):
    assert N >= 3
    return np.array([3, 2] + [1] * (N - 2), dtype=np.int64)


def fwd_operands(kind, D, N, H, seed=0):
    rs = np.random.RandomState(1000 * seed + 7 * D + N + H + GATES[kind])
    G = GATES[kind]
    return dict(kind=kind, D=D, N=N, H=H, lens=fwd_lens(N), Whh=weights(rs, D, G, H), bhh=rs.randint(-4, 5, (D, G * H)) / 16.0,
                GI=rs.randint(-8, 9, (TP * N, D * G * H)) / 8.0, h0=STATE_GRID[rs.randint(0, 6, (D, N, H))],
                c0=STATE_GRID[rs.randint(0, 6, (D, N, H))])


def fwd_first_step(op, d, Whh=None, h0=None):
    """Every sample's first processed step of direction d in float64: t [N], the state h (and c), the saved planes [N, NS*H] and the
    pre-activations.  Whh / h0 replace the case's own (the mutation helpers)."""
    kind, N, H, D = op["kind"], op["N"], op["H"], op["D"]
    G = GATES[kind]
    t = np.zeros(N, dtype=np.int64) if d == 0 else op["lens"] - 1
    gi = op["GI"].reshape(TP, N, D, G * H)[t, np.arange(N), d]
    W = op["Whh"][d] if Whh is None else Whh
    h = op["h0"][d] if h0 is None else h0
    gh = h @ W.T + op["bhh"][d]
    c = planes = None
    if kind == "gru":
        pr, pz = gi[:, :H] + gh[:, :H], gi[:, H:2 * H] + gh[:, H:2 * H]
        r, z, q = _sigmoid(pr), _sigmoid(pz), gh[:, 2 * H:]
        pn = gi[:, 2 * H:] + r * q
        n = np.tanh(pn)
        hn = (1 - z) * n + z * h
        planes, pre = np.concatenate([r, z, n, q], axis=1), np.concatenate([pr, pz, pn], axis=1)
    elif kind == "lstm":
        pre = gi + gh
        i, f, g, o = _sigmoid(pre[:, :H]), _sigmoid(pre[:, H:2 * H]), np.tanh(pre[:, 2 * H:3 * H]), _sigmoid(pre[:, 3 * H:])
        c = f * op["c0"][d] + i * g
        hn = o * np.tanh(c)
        planes = np.concatenate([i, f, g, o, c], axis=1)
    else:
        pre = gi + gh
        hn = np.tanh(pre)
    return dict(t=t, h=hn, c=c, planes=planes, pre=pre, gh=gh)


def fwd_budget(op, d):
    """Exact integer arithmetic: (the largest sum of term magnitudes of W_hh . h0 + GI + b_hh in units of 2^-10, True if the float64
    product equals the integer one)."""
    Wi, hi = np.rint(op["Whh"][d] * 256).astype(np.int64), np.rint(op["h0"][d] * 4).astype(np.int64)
    assert np.array_equal(Wi / 256.0, op["Whh"][d]) and np.array_equal(hi / 4.0, op["h0"][d])
    G, H, N, D = GATES[op["kind"]], op["H"], op["N"], op["D"]
    gi = np.rint(op["GI"].reshape(TP, N, D, G * H)[:, :, d] * 1024).astype(np.int64)
    bi = np.rint(op["bhh"][d] * 1024).astype(np.int64)
    assert np.array_equal(gi / 1024.0, op["GI"].reshape(TP, N, D, G * H)[:, :, d]) and np.array_equal(bi / 1024.0, op["bhh"][d])
    units = np.abs(hi) @ np.abs(Wi).T + np.abs(bi) + np.abs(gi).max(axis=0)
    same = np.array_equal((hi @ Wi.T) / 1024.0, op["h0"][d] @ op["Whh"][d].T)
    return int(units.max()), same


def swap_in_row(W, row, k1, k2):
    """A copy of W [G*H, H] (or [D, G*H, H] with row = (d, row)) with two elements of one row exchanged."""
    M = W.copy()
    r = M[row]
    r[k1], r[k2] = r[k2], r[k1]
    return M


def loudest_swap(op, d, row, n):
    """(k1, k2) of the row whose exchange moves sample n's pre-activation most: |W[k1] - W[k2]| * |h0[k1] - h0[k2]| is largest."""
    w, h = op["Whh"][d][row], op["h0"][d][n]
    eff = np.abs((w[:, None] - w[None, :]) * (h[:, None] - h[None, :]))
    k1, k2 = np.unravel_index(int(np.argmax(eff)), eff.shape)
    return int(k1), int(k2)


# ---- BPTT ----------------------------------------------------------------------------------------------------------------------------
def bwd_lens(N, state=False):
    """Half 3, half 2; with state (dh0 / dc0 of the launch-per-step BPTT) a third each of 3, 2 and 1."""
    assert N >= 3
    if not state:
        return np.array([3] * ((N + 1) // 2) + [2] * (N // 2), dtype=np.int64)
    n3 = (N + 2) // 3
    n2 = (N - n3 + 1) // 2
    return np.array([3] * n3 + [2] * n2 + [1] * (N - n3 - n2), dtype=np.int64)


def step_index(lens, d, which):
    """t of every sample's first (which = 0) or second (1) processed BPTT step of direction d."""
    return np.maximum(lens - 1 - which, 0) if d == 0 else np.full(len(lens), which, dtype=np.int64)


def bwd_operands(kind, D, N, H, seed=0, state=False, fp32=False):
    """dOut [T'][N][H], W_hh, hext [D][T'+2][N][H] (zero guard slots and padding, as the forward leaves them), the saved planes
    [D][T'][N][NS*H] (zero at padding), and with state the initial h0 / c0.  fp32: the storage type (LSTM: see the module's text)."""
    rs = np.random.RandomState(2000 * seed + 11 * D + N + H + GATES[kind])
    G, NS = GATES[kind], PLANES[kind]
    lens = bwd_lens(N, state)
    act = (np.arange(TP)[:, None] < lens[None, :]).astype(np.float64)[None, :, :, None]          # [1][T'][N][1]
    pick = lambda vals, *shape: np.asarray(vals, dtype=np.float64)[rs.randint(0, len(vals), shape)]
    op = dict(kind=kind, D=D, N=N, H=H, lens=lens, Whh=weights(rs, D, G, H), h0=None, c0=None, Sv=None,
              cmask=(np.arange(H)[None, :] + np.arange(N)[:, None]) % 3 == 0)
    op["dOut"] = pick([-1.0, 1.0] if kind == "lstm" else [-1.0, -0.5, 0.5, 1.0], TP, N, H)
    hext = np.zeros((D, TP + 2, N, H))
    hext[:, 1:TP + 1] = pick(STATE_GRID, D, TP, N, H) * act
    op["hext"] = hext
    if kind == "gru":
        planes = [np.full((D, TP, N, H), 0.5), pick([0.25, 0.5, 0.75], D, TP, N, H), pick([-0.5, 0.5], D, TP, N, H),
                  pick([-1.0, -0.5, 0.5, 1.0], D, TP, N, H)]
    elif kind == "lstm":
        c = pick([-0.75, -0.5, 0.5, 0.75], D, TP, N, H)
        for d in range(D):
            for which in (0, 1):
                t = step_index(lens, d, which)
                c[d, t, np.arange(N)] *= ~op["cmask"]
                if fp32 and which == 0:
                    c[d, t[1:], np.arange(1, N)] = 0.0
        half = np.full((D, TP, N, H), 0.5)
        planes = [half, half, pick([-0.5, 0.5], D, TP, N, H), half, c]
    if NS:
        op["Sv"] = np.concatenate(planes, axis=3) * act
    if state:
        op["h0"] = STATE_GRID[rs.randint(0, 6, (D, N, H))]
        if kind == "lstm":
            op["c0"] = STATE_GRID[rs.randint(0, 6, (D, N, H))]
    return op


def gate_grads(kind, H, dh, dc, P, hprev, cprev, hcur):
    """The gate-gradient formulas of one step (oracle.ds2_oracle.rnn_dir_bwd, csrc/ds2_rnn.hip k_rnn_step_bwd) for active samples:
    (dgi [N, G*H], hidden-side dgh [N, G*H], carried dh, carried dc)."""
    if kind == "gru":
        r, z, n, q = P[:, :H], P[:, H:2 * H], P[:, 2 * H:3 * H], P[:, 3 * H:]
        dn = dh * (1 - z) * (1 - n * n)
        dz = dh * (hprev - n) * z * (1 - z)
        dr = dn * q * r * (1 - r)
        return np.concatenate([dr, dz, dn], axis=1), np.concatenate([dr, dz, dn * r], axis=1), dh * z, None
    if kind == "lstm":
        i, f, g, o, c = (P[:, k * H:(k + 1) * H] for k in range(5))
        tc = np.tanh(c)
        dcn = dc + dh * o * (1 - tc * tc)
        dgi = np.concatenate([dcn * g * i * (1 - i), dcn * cprev * f * (1 - f), dcn * i * (1 - g * g), dh * tc * o * (1 - o)], axis=1)
        return dgi, dgi, np.zeros_like(dh), dcn * f
    dg = dh * (1 - hcur * hcur)
    return dg, dg, np.zeros_like(dh), None


def _step_inputs(op, d, t):
    """Planes, h_{t-1}, c_{t-1} and h_t of every sample at its step t[n] of direction d (forward order: t - 1 or t + 1; a sample's
    first forward step takes the initial state)."""
    kind, N, H, lens = op["kind"], op["N"], op["H"], op["lens"]
    ar = np.arange(N)
    tprev = t - 1 if d == 0 else t + 1
    has_prev = (t > 0) if d == 0 else (t + 1 < lens)
    zero = np.zeros((N, H))
    h0 = op["h0"][d] if op["h0"] is not None else zero
    c0 = op["c0"][d] if op["c0"] is not None else zero
    hprev = np.where(has_prev[:, None], op["hext"][d, 1 + tprev, ar], h0)
    P = cprev = None
    if op["Sv"] is not None:
        P = op["Sv"][d, t, ar]
        if kind == "lstm":
            cprev = np.where(has_prev[:, None], op["Sv"][d, np.clip(tprev, 0, TP - 1), ar][:, 4 * H:], c0)
    return P, hprev, cprev, op["hext"][d, 1 + t, ar]


def bwd_first_step(op, d):
    """Every sample's first processed BPTT step of direction d: no recurrent term, dh = dOut."""
    t = step_index(op["lens"], d, 0)
    P, hprev, cprev, hcur = _step_inputs(op, d, t)
    dh = op["dOut"][t, np.arange(op["N"])]
    dgi, dgh, ch, cc = gate_grads(op["kind"], op["H"], dh, np.zeros_like(dh), P, hprev, cprev, hcur)
    return dict(t=t, dgi=dgi, dgh=dgh, ch=ch, cc=cc)


def bwd_second_step(op, d, first, first_dgh, Whh=None):
    """The second processed step from the first step's hidden-side gate gradients AS GIVEN (first_dgh: what the device stored, or
    the reference's own) and the reference's elementwise carries.  absum: sum of the magnitudes of all terms of dh; gain_*: derivative
    of the outputs by dh (the formulas are linear in it)."""
    kind, N, H = op["kind"], op["N"], op["H"]
    W = op["Whh"][d] if Whh is None else Whh
    t = step_index(op["lens"], d, 1)                # samples of length 1 have no second step: their rows here mean nothing
    P, hprev, cprev, hcur = _step_inputs(op, d, t)
    dout = op["dOut"][t, np.arange(N)]
    prod = first_dgh @ W
    dh = dout + first["ch"] + prod
    absum = np.abs(first_dgh) @ np.abs(W) + np.abs(dout) + np.abs(first["ch"])
    dc = first["cc"] if first["cc"] is not None else np.zeros_like(dh)
    dgi, dgh, ch, cc = gate_grads(kind, H, dh, dc, P, hprev, cprev, hcur)
    ggi, ggh, _, gcc = gate_grads(kind, H, np.ones_like(dh), np.zeros_like(dh), P, hprev, cprev, hcur)
    return dict(t=t, dh=dh, dc=dc, prod=prod, absum=absum, dgi=dgi, dgh=dgh, ch=ch, cc=cc, gain_gi=np.abs(ggi), gain_gh=np.abs(ggh),
                gain_cc=None if gcc is None else np.abs(gcc), exact=exact_rows(first_dgh, absum), rows=op["lens"] >= 2)


def compared_units(op):
    """[N, H] units whose second-step outputs have an exact reference: all of them, for LSTM the cmask units."""
    return op["cmask"] if op["kind"] == "lstm" else np.ones((op["N"], op["H"]), dtype=bool)


def fp32_sum_bound(absum, K):
    """Rigorous bound of an fp32 sum of K terms in any order (each addition rounds once: (K - 1) * 2^-24 relative to the magnitudes)."""
    return K * 2.0 ** -24 * absum * 1.001


def oracle_cache(op, d):
    """The fabricated hext / planes as the cache oracle.ds2_oracle.rnn_dir_bwd expects (W_ih = identity)."""
    kind, N, H, lens = op["kind"], op["N"], op["H"], op["lens"]
    steps = []
    for t in (range(TP) if d == 0 else range(TP - 1, -1, -1)):
        tt = np.full(N, t, dtype=np.int64)
        P, hprev, cprev, hcur = _step_inputs(op, d, tt)
        st = dict(t=t, act=(t < lens)[:, None], hprev=hprev)
        if kind == "gru":
            st.update(r=P[:, :H], z=P[:, H:2 * H], n=P[:, 2 * H:3 * H], hn=P[:, 3 * H:])
        elif kind == "lstm":
            st.update(i=P[:, :H], f=P[:, H:2 * H], g=P[:, 2 * H:3 * H], o=P[:, 3 * H:4 * H], cprev=cprev, tc=np.tanh(P[:, 4 * H:]))
        else:
            st.update(hnew=hcur)
        steps.append(st)
    return dict(kind=kind, steps=steps, x=np.zeros((TP, N, GATES[kind] * H)), H=H)


# ---- the cases: (storage, cell, D, N, H, routing bits, kernel family).  Shapes from the lists tests/test_gpu_kernels.py runs ----------
# (three are not from there, because no listed shape reaches the place: family 2 needs 9-16 clips per group -- N = 64 with two
# directions, N = 128 with one -- and GRU-1280 with exactly 8 clips per group is N = 24)
F32, BF16 = "float32", "bfloat16"
# launch-per-step kernels (family 0: ops.PERSIST_ENABLED = False): k-tail at H = 48, four waves' chunks at 1024; one / two m-tiles
PER_STEP_CASES = [(dt, kind, D, N, H, 0, 0) for dt in (F32, BF16) for kind in ("gru", "lstm", "rnn")
                  for D, N, H in ((2, 3, 32), (1, 20, 48), (2, 37, 32), (2, {"gru": 11, "lstm": 13, "rnn": 9}[kind], 1024))]
# tuned H = 1024 kernels: family 1 (<= 8 clips per group), family 2 (9-16: the shipping route of the tanh cell, routing bit 16 for the others)
TUNED_CASES = [(BF16, "gru", 2, 11, 1024, 0, 1), (BF16, "gru", 1, 32, 1024, 0, 1), (BF16, "gru", 2, 32, 1024, 0, 1),
               (BF16, "lstm", 2, 13, 1024, 0, 1), (BF16, "lstm", 1, 5, 1024, 0, 1), (BF16, "rnn", 2, 9, 1024, 0, 1),
               (BF16, "gru", 2, 64, 1024, 16, 2), (BF16, "lstm", 2, 64, 1024, 16, 2), (BF16, "rnn", 2, 64, 1024, 0, 2),
               (BF16, "gru", 1, 128, 1024, 16, 2)]            # one direction: 16 clips in each of the eight groups
# round-2 general kernels (family 4): fp32 storage, and bf16 under routing bit 1; widths 800 / 1024 / 1280, one and four m-tiles
FAMILY4_CASES = [(F32, "gru", 2, 8, 800, 0, 4), (F32, "lstm", 1, 5, 800, 0, 4), (F32, "rnn", 1, 9, 800, 0, 4),
                 (F32, "gru", 2, 32, 1024, 0, 4), (F32, "lstm", 2, 3, 1024, 0, 4), (F32, "rnn", 2, 5, 1024, 0, 4),
                 (F32, "lstm", 1, 18, 1280, 0, 4), (F32, "gru", 2, 8, 1280, 0, 4), (F32, "rnn", 2, 12, 1280, 0, 4),
                 (BF16, "gru", 2, 8, 800, 1, 4), (BF16, "lstm", 2, 13, 800, 1, 4), (BF16, "gru", 2, 7, 1280, 1, 4),
                 (BF16, "lstm", 2, 64, 1280, 1, 4), (BF16, "gru", 2, 64, 1280, 1, 4)]
# round-4 general kernels (family 3): every instantiated width; from H = 1024 on (H % 256 == 0) both sides of the sparse-set rule
# (8 clips per group: structured-sparse products, 9: dense tiles); LSTM-1280 keeps a weight tail in LDS
FAMILY3_CASES = [(BF16, "gru", 2, 9, 384, 0, 3), (BF16, "gru", 2, 3, 512, 0, 3), (BF16, "lstm", 1, 100, 512, 0, 3),
                 (BF16, "gru", 2, 33, 640, 0, 3), (BF16, "gru", 1, 20, 768, 0, 3), (BF16, "lstm", 2, 13, 800, 0, 3),
                 (BF16, "gru", 1, 7, 896, 0, 3), (BF16, "gru", 2, 96, 1024, 0, 3), (BF16, "lstm", 2, 64, 1024, 0, 3),
                 (BF16, "lstm", 2, 11, 1152, 0, 3), (BF16, "lstm", 2, 24, 1280, 0, 3), (BF16, "gru", 2, 27, 1280, 0, 3),
                 (BF16, "lstm", 1, 3, 1280, 0, 3), (BF16, "lstm", 2, 64, 1280, 0, 3), (BF16, "gru", 2, 16, 1408, 0, 3),
                 (BF16, "gru", 1, 9, 1536, 0, 3), (BF16, "gru", 2, 30, 1536, 0, 3),
                 # the sparse-set rule within one cell: GRU-1280 with 3 and 8 clips per group (sparse) next to 9 above (dense), LSTM-1280
                 # with 11 (dense) next to 8 above; H = 1024 sends <= 8 clips to the tuned kernels, so its sparse instantiation runs
                 # under routing bit 8
                 (BF16, "gru", 2, 7, 1280, 0, 3), (BF16, "gru", 2, 24, 1280, 0, 3), (BF16, "lstm", 2, 32, 1280, 0, 3),
                 (BF16, "gru", 2, 32, 1024, 8, 3), (BF16, "lstm", 2, 32, 1024, 8, 3)]
ALL_CASES = PER_STEP_CASES + TUNED_CASES + FAMILY4_CASES + FAMILY3_CASES


def case_id(c):
    return "%s-%s-D%d-N%d-H%d-v%d-f%d" % c
