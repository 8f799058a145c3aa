"""The small streaming kernels of csrc/ds2_seqops.hip that the other kernel tests reach only through a GEMM or a whole model: the bias
gradient plane map, the hi/lo split of fp32 operands (vector path, scalar tail, zero fill, row-stacked segments), the padding-row
zeroing with a padded stride, the grid-stride wrap of the element-wise kernels (ew_grid caps at 2048 blocks of 256 threads,
ds2_copy_words at 256), and softmax_rows beyond its one model shape.  References are plain torch / numpy expressions."""
import ctypes as C

import numpy as np
import pytest
import torch

from fixtures import DEV, cu, np64, relerr

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
EW_CAP = 2048 * 256      # threads of a capped ew_grid launch: one more element forces a second grid-stride trip
SENTINEL = 7.0


def ops():
    from deepspeech.pytorch_amd import ops as _ops
    return _ops


def bits(t):
    """the storage words of a tensor (NaN-safe equality)"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gru", "lstm", "rnn"])
@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("N,H", [(1, 8), (5, 40), (33, 300)])      # (33, 300): D * NB * H is no multiple of the 256-thread block
def test_rnn_bias_grads_plane_map(kind, D, N, H):
    """bias_ih.grad = planes 0..G-1 of the per-sample sums; bias_hh.grad the same, except GRU: planes 0, 1, 3 (the hidden side's n slot is
    dq = dn * r, plane 2 = dn belongs to bias_ih only)."""
    o = ops()
    G = {"gru": 3, "lstm": 4, "rnn": 1}[kind]
    NB = 4 if kind == "gru" else G
    rs = np.random.RandomState(100 * D + N)
    bacc = rs.standard_normal((D, N, NB * H)).astype(np.float32)
    s = bacc.astype(np.float64).sum(1).reshape(D, NB, H)              # [D][plane][unit]
    ref_ih = s[:, :G].reshape(D * G * H)
    ref_hh = (s[:, [0, 1, 3]] if kind == "gru" else s[:, :G]).reshape(D, G * H)
    dbih, dbhh = o.rnn_bias_grads(kind, cu(bacc), D, N, H)
    assert dbih.shape == (D * G * H,) and dbhh.shape == (D, G * H)
    assert relerr(np64(dbih), ref_ih) < 1e-6
    assert relerr(np64(dbhh), ref_hh) < 1e-6
    if kind == "gru":
        third = np64(dbhh).reshape(D, 3, H)[:, 2]
        assert relerr(third, s[:, 3]) < 1e-6
        assert np.abs(third - s[:, 2]).max() > 1e-2 * np.abs(s[:, 2]).max()


# ---------------------------------------------------------------------------------------------------------------
def _split_source(rows, K, seed):
    """(window, hi, lo): a [rows][K] column window (row stride > K, more columns behind it) of a wider fp32 matrix with rows of very
    different scale, and its bf16 halves hi = bf16(x), lo = bf16(x - hi)."""
    rs = np.random.RandomState(seed)
    wide = rs.standard_normal((rows, (K + 3) // 4 * 4 + 12)) * np.exp(rs.uniform(-3, 3, (rows, 1)))
    wide = cu(wide)
    X = wide[:, 4:4 + K]
    assert X.stride(0) > K and X.data_ptr() % 16 == 0
    hi = X.to(torch.bfloat16)
    lo = (X - hi.float()).to(torch.bfloat16)
    return X, hi, lo


@pytest.mark.parametrize("rows", [1, 37])
@pytest.mark.parametrize("K", [64, 100, 333, 808])     # K % 8 = 0, 4, 5, 0: whole 16-byte chunks only / a scalar tail of 4 / of 5
def test_split3_segments_are_bit_exact(rows, K):
    o = ops()
    X, hi, lo = _split_source(rows, K, K + rows)
    assert lo.float().abs().max() > 0
    Kp = (K + 63) // 64 * 64
    for mode, segs in ((0, (hi, hi, lo)), (1, (hi, lo, hi))):
        got = o.split3(X, mode)
        assert got.shape == (rows, 3 * Kp) and got.dtype == torch.bfloat16
        for i, seg in enumerate(segs):
            assert torch.equal(got[:, i * Kp:i * Kp + K], seg), (mode, i)
            assert not got[:, i * Kp + K:(i + 1) * Kp].any(), (mode, i)          # zero fill of [K, Kp)
    K8 = (K + 7) // 8 * 8
    for mode, segs in ((0, (hi, hi, lo)), (1, (hi, lo, hi))):
        got = o.split3_rows(X, mode)
        assert got.shape == (3 * rows, K8)
        for i, seg in enumerate(segs):
            assert torch.equal(got[i * rows:(i + 1) * rows, :K], seg), (mode, i)
            assert not got[i * rows:(i + 1) * rows, K:].any(), (mode, i)


def test_split3_into_a_row_window_leaves_the_other_rows():
    o = ops()
    rows, K, Kp = 37, 100, 128
    X, hi, lo = _split_source(rows, K, 3)
    buf = torch.full((rows + 6, 3 * Kp), SENTINEL, dtype=torch.bfloat16, device=DEV)
    o.split3(X, 1, out=buf[3:3 + rows])
    assert bool((buf[:3] == SENTINEL).all()) and bool((buf[3 + rows:] == SENTINEL).all())
    win = buf[3:3 + rows]
    assert torch.equal(win[:, :K], hi) and torch.equal(win[:, Kp:Kp + K], lo) and torch.equal(win[:, 2 * Kp:2 * Kp + K], hi)
    assert not win[:, K:Kp].any() and not win[:, Kp + K:2 * Kp].any() and not win[:, 2 * Kp + K:].any()


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Tp,N,cols,ld,lens", [
    (5, 3, 8, 8, [2, 5, 1]),                              # R = 15 is no multiple of the 4 rows of a workgroup
    (37, 8, 264, 320, [20, 37, 1, 36, 5, 18, 37, 9]),     # ld > cols: the pad columns of a padding row stay
    (9, 1, 1344, 1344, [9]),                              # a row longer than one pass of the 64 lanes; nothing to zero
    (9, 3, 1344, 1344, [4, 9, 2]),                        # the same width with padding rows
])
def test_zero_pad_rows_touches_only_the_padding(dtype, Tp, N, cols, ld, lens):
    rs = np.random.RandomState(Tp + N)
    R = Tp * N
    buf = torch.full((R, ld), SENTINEL, dtype=dtype, device=DEV)
    buf[:, :cols] = cu(rs.standard_normal((R, cols)), dtype)
    live = (torch.arange(Tp)[:, None] < torch.tensor(lens)[None, :]).reshape(R).to(DEV)      # row t * N + n
    assert max(lens) == Tp and (N == 1 or lens not in (sorted(lens), sorted(lens, reverse=True)))
    buf[:, :cols][~live] = float("nan")
    before = buf.clone()
    out = ops().zero_pad_rows(buf[:, :cols], torch.tensor(lens, dtype=torch.int32, device=DEV), Tp, N)
    assert out.data_ptr() == buf.data_ptr()
    assert torch.equal(bits(buf[live]), bits(before[live]))
    assert not bits(buf[:, :cols][~live]).any()
    assert bool((buf[:, cols:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nvec", [1, EW_CAP + 3])
def test_add2_wraps_its_grid_bit_exactly(dtype, nvec):
    n = nvec * (4 if dtype == torch.float32 else 8)
    gen = torch.Generator(device=DEV).manual_seed(1)
    a, b = (torch.randn(n, device=DEV, generator=gen).to(dtype) for _ in range(2))
    assert torch.equal(ops().add2(a, b), (a.float() + b.float()).to(dtype))


@pytest.mark.parametrize("n,slices", [(4, 3), (4 * (EW_CAP + 5), 3), (4 * (EW_CAP + 5), 1)])
def test_sum_slices_wraps_its_grid_in_index_order(n, slices):
    from deepspeech.pytorch_amd.ops import P, S
    from deepspeech.pytorch_amd._lib import call
    gen = torch.Generator(device=DEV).manual_seed(2)
    src = torch.randn((slices, n), device=DEV, generator=gen) * torch.tensor([1.0, 1e3, 1e-3], device=DEV)[:slices, None]
    out = torch.full((n + 4,), SENTINEL, device=DEV)
    call("ds2_sum_slices", P(src), P(out), n, slices, S())
    ref = src[0].clone()
    for s in range(1, slices):
        ref = ref + src[s]                      # left to right: ((s0 + s1) + s2)
    assert torch.equal(out[:n], ref) and bool((out[n:] == SENTINEL).all())


@pytest.mark.parametrize("n", [5, EW_CAP + 77])
def test_scale_by_wraps_its_grid_bit_exactly(n):
    gen = torch.Generator(device=DEV).manual_seed(3)
    buf = torch.randn(n + 3, device=DEV, generator=gen)
    ref, s = buf.clone(), torch.tensor([0.3712], device=DEV)
    ops().scale_by_(buf[:n], s)
    assert torch.equal(buf[:n], ref[:n] * s) and torch.equal(buf[n:], ref[n:])


def test_copy_words_wraps_its_grid_and_accepts_zero_words():
    from deepspeech.pytorch_amd.ops import P, S
    from deepspeech.pytorch_amd._lib import call
    n = 256 * 256 + 9                           # 256 blocks of 256 threads: 9 words are left for a second trip
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int32, device=DEV)
    dst = torch.full((n + 5,), 7, dtype=torch.int32, device=DEV)
    call("ds2_copy_words", P(src), P(dst), n, S())
    assert torch.equal(dst[:n], src) and bool((dst[n:] == 7).all())
    dst.fill_(7)
    call("ds2_copy_words", P(src), P(dst), 0, S())          # raises on a non-zero status
    call("ds2_copy_words", C.c_void_p(0), C.c_void_p(0), 0, S())
    assert bool((dst == 7).all())


# ---------------------------------------------------------------------------------------------------------------
def _softmax_case(rows, Cc):
    rs = np.random.RandomState(13 + Cc)
    x = rs.standard_normal((rows, Cc)) * 4
    if Cc > 1:
        x[0] = -40 + 0.1 * rs.standard_normal(Cc)             # a spread of 80 in one row: exp() needs the max subtracted
        x[0, Cc // 2] = 40
    x = x.astype(np.float32).astype(np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    ref = e / e.sum(-1, keepdims=True)
    ld = (Cc + 31) // 32 * 32
    lg = torch.full((rows, ld), 1e30, dtype=torch.float32, device=DEV)       # pad columns must not be read into the max
    lg[:, :Cc] = cu(x)
    p = np64(ops().softmax_rows(lg, Cc))
    assert p.shape == (rows, Cc)
    e_p, e_sum = np.abs(p - ref).max(), np.abs(p.sum(-1) - 1).max()
    print("max |p - ref| %.3e   max |row sum - 1| %.3e" % (e_p, e_sum))
    assert e_p < 1e-6
    assert e_sum < 1e-6


@pytest.mark.parametrize("rows", [1, 77])
@pytest.mark.parametrize("Cc", [1, 29, 32, 257])
def test_softmax_rows_widths_and_padded_logits(rows, Cc):
    _softmax_case(rows, Cc)


def test_softmax_rows_wraps_its_grid():
    _softmax_case(EW_CAP + 77, 29)
