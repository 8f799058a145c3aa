"""Operands, float64 references, expected bits and tile arithmetic of the exact conv tests (tests/test_gpu_conv_exact.py on the
device, tests/test_conv_exact_host.py without one).

Every conv kernel of csrc/ds2_conv.hip is linear, multiplies bf16 or fp32 operands and adds in fp32.  With small INTEGER operands
every product and every partial sum is an integer below 2^24, so every fp32 addition is exact whatever the tile order, K-split,
cross-wave reduction or partial-sum workspace: the fp32 result IS the mathematical result.  An fp32 output therefore has to equal
the float64 reference in every element, and a bf16 output its round-to-nearest-even bf16 (one rounding: the fp32 value is exact).
No tolerance, no exempted element.

Reference: float64 torch.nn.functional.conv2d on the CPU and its autograd (pinned to oracle.conv2d_fwd / conv2d_bwd by the host
test).  Operands come from a seeded CPU torch.Generator and are masked as the pipeline masks them: conv1's input is zero beyond
each clip's input length, conv2's input and every output gradient are zero at t >= lens[n]; the forward output is masked at
t >= lens[n]; conv2's dX is taken at ALL positions (the formula at ds2_conv2_dgrad)."""
import torch

from oracle import ds2_oracle as O

EXACT = 1 << 24
CONV1 = dict(stride=(2, 2), padding=(20, 5), kernel=(41, 11))
CONV2 = dict(stride=(2, 1), padding=(10, 5), kernel=(21, 11))
CH = 32
CUS_OF_THE_TABLES = 256


# ---- geometry and tile arithmetic (plain restatements of the launch code) -----------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def conv_rows(F0):
    F1 = (F0 + 2 * 20 - 41) // 2 + 1
    return F1, (F1 + 2 * 10 - 21) // 2 + 1


def out_frames(T):
    """T' of both layers for T input frames (conv1 halves the time axis, conv2 keeps it)."""
    return (T - 1) // 2 + 1


def rtap_tiles(N, Tp, U):
    """k_conv_rtap: tiles of 4 output rows x 32 frames.  Forward: U = 41 on both launches; dgrad: U = 41 (even rows), 40 (odd rows)."""
    return N * cdiv(U, 4) * cdiv(Tp, 32)


def conv1_mfma_tiles(N, Tp):
    """k_conv1_fwd_mfma / k_conv1_wgrad_mfma: blocks of 9 output rows x 128 frames, 9 row blocks."""
    return N * cdiv(Tp, 128) * 9


C1W_MAXBLOCKS = 1024


def conv1_wgrad_chunks(N, F1, Tp):
    """k_conv1_wgrad<T>: chunks of 4 output rows x 64 frames on at most C1W_MAXBLOCKS workgroups."""
    return N * cdiv(F1, 4) * cdiv(Tp, 64)


CWR_SPLITS, CWD_TB, CWD_NJ = 85, 112, 44


def wgrad_bf16d_items(N, Tp):
    """k_conv2_wgrad_bf16d: work items (sample, j in [0, 44), tile of 112 positions), every 85th one to a split."""
    return N * CWD_NJ * cdiv(Tp, CWD_TB)


def regime(tiles, workgroups):
    """How a persistent launch of min(tiles, workgroups) workgroups walks `tiles` with tile += gridDim.x:
    "one"   every workgroup does a single tile (and takes the "no next tile" path behind it),
    "two"   some workgroups take a second tile, the others do not,
    "three" every workgroup takes a second tile and some a third (patch buffers 0 -> 1 -> 0),
    "other" anything else (exactly two tiles each, or more than three)."""
    if tiles <= workgroups:
        return "one"
    if tiles < 2 * workgroups:
        return "two"
    if 2 * workgroups < tiles <= 3 * workgroups:
        return "three"
    return "other"


def rtap_regimes(N, Tp, cus):
    """Regimes of the three distinct k_conv_rtap launch shapes of a conv2 forward + dgrad (U = 41 for both forward launches and the
    even dgrad rows, U = 40 for the odd dgrad rows)."""
    return {regime(rtap_tiles(N, Tp, U), cus) for U in (41, 40)}


def conv1_mfma_regimes(N, Tp, cus):
    return {regime(conv1_mfma_tiles(N, Tp), cus)}


def batch_for(regimes_of, want, Tp, cus, n256):
    """The batch size that puts a persistent kernel into regime `want` at T' = Tp on a device with `cus` compute units: the table's
    own N on 256 CUs, otherwise the N closest to it in proportion to the CU count that reaches the regime (None when there is none).
    The single-tile cases keep their N: their batch is what their lengths need, and the largest of them is 88 tiles."""
    if cus == CUS_OF_THE_TABLES or want == "one":
        return n256
    target = n256 * cus / CUS_OF_THE_TABLES
    for N in sorted(range(1, 4 * n256 * cdiv(cus, CUS_OF_THE_TABLES) + 2), key=lambda n: (abs(n - target), n)):
        if regimes_of(N, Tp, cus) == {want}:
            return N
    return None


# ---- the tables (N as on 256 CUs) ---------------------------------------------------------------------------------------------
# conv2, bf16, 161 bins: k_conv_rtap<11>, <10>, k_conv2_wgrad_bf16d.  (N, T', rtap regime)
CONV2_BF16 = [
    (1, 1, "one"),       # one frame, narrower than the 5-frame halo; wgrad: 44 items for 85 splits, the idle splits write zeros
    (2, 33, "one"),      # one frame into a second frame tile
    (2, 112, "one"),     # the wgrad tile of 112 positions: exact fit ...
    (2, 113, "one"),     # ... and a second tile holding a single position
    (3, 257, "two"),     # 297 / 270 tiles: a second tile for some workgroups, "no next tile" for the others; last frame tile: 1 frame
    (6, 289, "three"),   # 660 / 600 tiles: buffers 0 -> 1 -> 0; last frame tile: 1 frame; wgrad: 3 tiles per row, carries in t, j, n
]
# conv1, bf16, 161 bins: k_conv1_fwd_mfma, k_conv1_wgrad_mfma.  (N, T, regime)
CONV1_BF16 = [
    (1, 1, "one"),       # smallest input
    (2, 255, "one"),     # T' = 128: the 128-frame block, exact fit (odd T)
    (2, 256, "one"),     # T' = 128 (even T)
    (2, 257, "one"),     # T' = 129: a second block of one frame
    (8, 1025, "two"),    # T' = 513: 360 tiles, a second tile for some workgroups; the last block has 1 frame
    (12, 1537, "three"),  # T' = 769: 756 tiles, three per workgroup
]
# fp32 at 161 bins, N = 2: k_conv1_fwd<float> / k_conv1_wgrad<float> (64-frame tile), k_conv_tap<float, 1> forward (32),
# k_conv_tap<float, 2> dgrad (64), k_conv2_wgrad<float> (CW_TB = 128)
CONV1_F32_T = [127, 129]                   # T' = 64, 65
CONV2_F32_TP = [32, 33, 64, 65, 129]
# other geometries, fp32 and bf16 (the general kernels in both storage types): one shape each, N = 2, T' = 40.
# F0 = 9: F1 = 5, F2 = 3 -- fewer rows than a 4-row tile and than the kernel height; F1 odd: dgrad covers 3 even and 2 odd rows
OTHER_F0 = [81, 41, 257, 9]
OTHER_N, OTHER_T, OTHER_TP = 2, 80, 40
# k_conv1_wgrad<T>'s chunk loop past its cap of 1 024 blocks.  (dtype name, F0, N, T, chunks)
CONV1_CHUNK_LOOP = [("float32", 161, 4, 1537, 1092), ("bfloat16", 81, 8, 1537, 1144)]


def all_conv1_cases():
    """(F0, N, T) of every conv1 case of the tables (N as on 256 CUs)."""
    return ([(161, N, T) for N, T, _ in CONV1_BF16] + [(161, 2, T) for T in CONV1_F32_T] + [(F0, OTHER_N, OTHER_T) for F0 in OTHER_F0] +
            [(F0, N, T) for _, F0, N, T, _ in CONV1_CHUNK_LOOP])


def all_conv2_cases():
    """(F0, N, T') of every conv2 case of the tables (N as on 256 CUs)."""
    return ([(161, N, Tp) for N, Tp, _ in CONV2_BF16] + [(161, 2, Tp) for Tp in CONV2_F32_TP] + [(F0, OTHER_N, OTHER_TP) for F0 in OTHER_F0])


# ---- lengths and operands -----------------------------------------------------------------------------------------------------
def out_lens(N, Tp):
    """Output lengths of a batch, as far as N goes in this order: a clip of full length, one ending exactly on a 32-frame tile seam
    (the last seam below T'), one ending one frame past it (the full-length clip itself when T' = seam + 1), one of length 1; any
    further clip 41 frames shorter than the one before.  Sorted, longest first."""
    seam = 32 * ((Tp - 1) // 32)
    lens = []
    for c in (Tp, seam, seam + 1, 1):
        if 1 <= c <= Tp and c not in lens:
            lens.append(c)
    k = 1
    while len(lens) < N:
        lens.append(max(1, Tp - 41 * k))
        k += 1
    return sorted(lens[:N], reverse=True)


def ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64).to(torch.float64)


def time_mask(lens, Tp):
    """[N][T'] float64: 1 where t < lens[n]."""
    return (torch.arange(Tp)[None, :] < torch.as_tensor(lens)[:, None]).to(torch.float64)


def conv1_operands(F0, N, T, seed=None):
    """x (N,1,F0,T) and w (32,1,41,11) in {-2..2}, b in {-4..4}, dy (N,32,F1,T') in {-1,0,1}; x zero beyond lens_in, dy at t >= lens."""
    g = torch.Generator().manual_seed(1000 + 7 * T + N + F0 if seed is None else seed)
    F1, Tp = conv_rows(F0)[0], out_frames(T)
    want = out_lens(N, Tp)
    lens_in = [T if L == Tp else 2 * L - 1 for L in want]          # the shortest input that gives L output frames; the full clip: T
    lens = O.seq_lens(lens_in)
    assert lens.tolist() == want and int(O.seq_lens([T])[0]) == Tp
    x = ints(g, -2, 2, (N, 1, F0, T)) * time_mask(lens_in, T)[:, None, None, :]
    w, b = ints(g, -2, 2, (CH, 1) + CONV1["kernel"]), ints(g, -4, 4, (CH,))
    dy = ints(g, -1, 1, (N, CH, F1, Tp)) * time_mask(lens, Tp)[:, None, None, :]
    return dict(layer=CONV1, F0=F0, N=N, T=T, Tp=Tp, lens_in=lens_in, lens=lens, x=x, w=w, b=b, dy=dy)


def conv2_operands(F0, N, Tp, seed=None):
    """a1 (N,32,F1,T'), w (32,32,21,11) and dy (N,32,F2,T') in {-1,0,1}, b in {-4..4}; a1 and dy zero at t >= lens."""
    g = torch.Generator().manual_seed(2000 + 7 * Tp + N + F0 if seed is None else seed)
    F1, F2 = conv_rows(F0)
    lens = O.seq_lens([2 * L - 1 for L in out_lens(N, Tp)])         # through the oracle's length rule, as the pipeline gets them
    assert lens.tolist() == out_lens(N, Tp)
    m = time_mask(lens, Tp)[:, None, None, :]
    x = ints(g, -1, 1, (N, CH, F1, Tp)) * m
    w, b = ints(g, -1, 1, (CH, CH) + CONV2["kernel"]), ints(g, -4, 4, (CH,))
    dy = ints(g, -1, 1, (N, CH, F2, Tp)) * m
    return dict(layer=CONV2, F0=F0, N=N, T=Tp, Tp=Tp, lens=lens, x=x, w=w, b=b, dy=dy)


# ---- references ---------------------------------------------------------------------------------------------------------------
def assert_exact(name, v):
    """Every value an integer below 2^24: fp32 sums of it and towards it are exact.  Returns it without negative zeros."""
    assert v.dtype == torch.float64
    assert bool((v == v.round()).all()), name + ": a reference value is not an integer"
    big = float(v.abs().max()) if v.numel() else 0.0
    assert big < EXACT, "%s: |reference| reaches %g, not below 2^24" % (name, big)
    return v + 0.0


def reference(case, need_dx):
    """float64 conv2d and its autograd.  y (N,32,F',T') masked at t >= lens, dw (32,C,KF,KT), dx like x (or None): all integers
    below 2^24, asserted."""
    x = case["x"].clone().requires_grad_(need_dx)
    w = case["w"].clone().requires_grad_(True)
    y = torch.nn.functional.conv2d(x, w, case["b"], stride=case["layer"]["stride"], padding=case["layer"]["padding"])
    assert tuple(y.shape) == tuple(case["dy"].shape)
    y.backward(case["dy"])
    live = time_mask(case["lens"], case["Tp"])[:, None, None, :] > 0
    ym = torch.where(live, y.detach(), torch.zeros((), dtype=torch.float64))
    return dict(y=assert_exact("y", ym), dw=assert_exact("dw", w.grad), dx=assert_exact("dx", x.grad) if need_dx else None)


# ---- layouts (the expressions of tests/test_gpu_kernels.py) and expected bits --------------------------------------------------
def nftc(a):
    """(N,C,F,T) -> [N][F][T][C]"""
    return a.permute(0, 2, 3, 1).contiguous()


def conv1_weight_layout(w):
    """(32,1,41,11) -> w1k [451][32]; the layout of conv1's dW too"""
    return w.reshape(CH, 451).T.contiguous()


def conv2_weight_layout(w):
    """(32,32,21,11) -> w2t [kf][kt][co][ci]; as [231][32][32] the layout of conv2's dW"""
    return w.permute(2, 3, 0, 1).contiguous()


def conv2_dgrad_weight_layouts(w):
    """the flipped parity sub-kernels [M_q * 11][ci][co] of the data gradient, q = 0, 1"""
    return [w[:, :, q::2, :].flip(2, 3).permute(2, 3, 1, 0).contiguous() for q in (0, 1)]


def expected(v, dtype):
    """The exact value as the kernel has to store it: float32 (exact), then for bf16 storage ONE round-to-nearest-even."""
    f = v.to(torch.float32)
    assert bool((f.to(torch.float64) == v).all())
    return f if dtype == torch.float32 else f.to(torch.bfloat16)


def words(t):
    """the storage words of a float32 / bfloat16 tensor"""
    return t.contiguous().view({torch.float32: torch.int32, torch.bfloat16: torch.int16}[t.dtype])


def mismatch(got, want):
    """None when the two tensors agree in every storage word, otherwise a report: how many differ, the first index, got / want."""
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    got, want = got.cpu(), want.cpu()
    if torch.equal(words(got), words(want)):
        return None
    bad = (words(got) != words(want)).nonzero()
    first = tuple(bad[0].tolist())
    return "%d of %d elements differ; first at %s: got %r, want %r" % (len(bad), got.numel(), first, float(got[first]), float(want[first]))
