"""Torch-tensor wrappers around the C ABI (include/ds2hip.h).  torch is used here only as the owner of device
memory and streams; every computation is a ds2hip kernel.  All tensors must be CUDA(HIP) tensors -- there is no CPU
path (a CPU tensor raises)."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import F32, BF16, call, query

CELLS = {"gru": _lib.CELL_GRU, "lstm": _lib.CELL_LSTM, "rnn": _lib.CELL_RNN_TANH}
GATES = {"gru": 3, "lstm": 4, "rnn": 1}
SAVED_PLANES = {"gru": 4, "lstm": 5, "rnn": 0}


def dt(t):
    d = t if isinstance(t, torch.dtype) else t.dtype
    if d == torch.float32:
        return F32
    if d == torch.bfloat16:
        return BF16
    raise TypeError("ds2hip supports float32 and bfloat16 activations, got %s" % d)


def vecw(dtype):
    return 4 if dtype == torch.float32 else 8


def P(t):
    """device pointer of a tensor (None -> NULL); refuses CPU tensors: the HIP path is the only path."""
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise _lib.Ds2HipError("ds2hip ops need CUDA(HIP) tensors; got a %s tensor -- there is no CPU fallback" % t.device)
    return C.c_void_p(t.data_ptr())


def PF(t):
    """device pointer of an fp32 parameter / buffer / statistics tensor.  The kernels read these as float: a module cast with
    .half() / .to(bfloat16) (or a 'bf16-true' precision plugin) must fail loudly instead of being read as garbage."""
    if t is not None and t.dtype != torch.float32:
        raise _lib.Ds2HipError("ds2hip kernels keep parameters, BatchNorm statistics and carried states in float32 (bf16 is an "
                               "activation/operand type selected by `precision`/autocast); got %s" % t.dtype)
    return P(t)


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rup(x, m):
    return (x + m - 1) // m * m


# Optional measurement hook (bench.py): when set to a list, every recurrent sweep appends
# (tag, n_launches, start_event, end_event) recorded on the stream the kernels are launched on.
SWEEP_EVENTS = None


class _sweep_timer:
    def __init__(self, tag, launches):
        self.tag, self.launches = tag, launches

    def __enter__(self):
        if SWEEP_EVENTS is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if SWEEP_EVENTS is not None:
            self.e1.record()
            SWEEP_EVENTS.append((self.tag, self.launches, self.e0, self.e1))
        return False


# ---------------------------------------------------------------------------------------------------------------
def pad_ld(n, dtype=torch.bfloat16):
    """Leading dimension for a matrix with n columns that the large GEMMs stream by rows: a row stride that is a multiple of
    1 KiB maps every row of a tile onto the same few memory channels (measured: the K = 1024 input projection runs 714 TFLOP/s
    with ld 1024 and 800-846 with ld 1088 / 1152, profiles/r03b_gemm8_ld.txt) -- such widths get 64 extra columns."""
    esz = 2 if dtype == torch.bfloat16 else 4
    return n + 64 if (n * esz) % 1024 == 0 else n


def empty_padded(rows, cols, dtype, device):
    """[rows][cols] view (row stride pad_ld(cols)) of a fresh allocation."""
    ld = pad_ld(cols, dtype)
    return torch.empty((rows, ld), dtype=dtype, device=device)[:, :cols] if ld != cols else torch.empty((rows, cols), dtype=dtype, device=device)


GEMM8_ENABLED = True     # tests flip this to run the 128x128-tile kernels on shapes the 256x256 kernel covers


def gemm8_nt_shape_ok(dtype, M, N, K, lda, ldb):
    """The shape part of gemm8_nt_ok (decidable before the operands exist)."""
    return (GEMM8_ENABLED and dtype == torch.bfloat16 and K % 64 == 0 and lda % 8 == 0 and ldb % 8 == 0 and
            M >= 1024 and N >= 256 and rup(M, 256) // 256 * (rup(N, 256) // 256) >= 160 and M * lda < (1 << 31) and N * ldb < (1 << 31))


def gemm8_nt_ok(A, B, M, N, K, lda, ldb):
    """Shapes the 256x256 phase-split kernel takes (and wins on): bf16, whole K-tiles, enough tiles to fill the chip."""
    return (A.dtype == B.dtype and gemm8_nt_shape_ok(A.dtype, M, N, K, lda, ldb) and
            A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0)


def wgrad_tn_ok(dtype, R, M, N, lda=None, ldb=None):
    """Weight gradients as grouped TN products (no operand transposes): bf16 activations, a long contraction, 8-aligned widths, and
    operands whose R x ld elements stay inside the kernels' 32-bit offsets (ds2_gemm8_tn_grouped / _wgrad_dx require K * ld < 2^31:
    beyond it -- e.g. R = T'N = 256 000 rows of a BiLSTM-1280's dGI, ld 10 240 -- the transpose + NT path takes over)."""
    lda = M if lda is None else lda
    ldb = N if ldb is None else ldb
    return (GEMM8_ENABLED and dtype == torch.bfloat16 and R >= 512 and M % 8 == 0 and N % 8 == 0 and M >= 256 and N >= 256 and
            R * lda < (1 << 31) and R * ldb < (1 << 31))


def zero_pad_rows(X, lens, Tp, N):
    """X[(t*N + n)][:] = 0 for t >= lens[n]: the rows a row-list product leaves unwritten."""
    call("ds2_zero_pad_rows", dt(X), P(X), X.stride(0), X.shape[1], P(lens), Tp, N, S())
    return X


def gemm_nt(A, B, bias=None, out_dtype=None, M=None, N=None, K=None, lda=None, ldb=None, out=None, ldc=None, splitk=1,
            batch=1, sA=0, sB=0, sC=0, sBias=0, coresident=False, rows=None, zero_pad=None):
    """C[M][N] = A[M][K] * B[N][K]^T (+bias).  A, B: 2-D row-major tensors (or explicit M/N/K/ld for views).
    rows (int32 device tensor or None): on the 256x256 kernel only the listed rows of A / C are visited (the frames of a padded
    sequence matrix that pack_padded_sequence keeps, model.py:96); zero_pad = (lens, Tp, N): the other rows of C are then zero,
    without it they are unspecified (unwritten by the 256x256 kernel; the kernels without row lists compute every row)."""
    M = A.shape[-2] if M is None else M
    N = B.shape[-2] if N is None else N
    K = A.shape[-1] if K is None else K
    lda = A.stride(-2) if lda is None else lda
    ldb = B.stride(-2) if ldb is None else ldb
    out_dtype = out_dtype or A.dtype
    if out is None and splitk == 1 and batch == 1 and not coresident and gemm8_nt_ok(A, B, M, N, K, lda, ldb):
        res = gemm8_nt(A, B, bias=bias, out_dtype=out_dtype, M=M, N=N, K=K, lda=lda, ldb=ldb, rows=rows)
        if rows is not None and zero_pad is not None:
            zero_pad_rows(res, *zero_pad)
        return res
    ks = fp32_ksplit(A.dtype, M, N, K) if (out is None and splitk == 1 and batch == 1 and not coresident and bias is None and
                                            out_dtype == torch.float32 and A.dtype == torch.float32) else 1
    if ks > 1:
        # fp32 mode, few output tiles and a long contraction (a layer's dX at config 2: 49 tiles of K = 4 800 on 256 CUs): the
        # K-slices run as the kernel's BATCH into a [slices][M][N] scratch and are added in index order (ds2_sum_slices) -- split-K
        # without atomics, i.e. with a fixed summation order
        Ks = K // ks
        ws = torch.empty((ks, M, N), dtype=torch.float32, device=A.device)
        call("ds2_gemm_nt", dt(A), P(A), P(B), P(ws), None, M, N, Ks, lda, ldb, N, 1, ks, Ks, Ks, M * N, 0, 1, S())
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
        call("ds2_sum_slices", P(ws), P(out), M * N, ks, S())
        if rows is not None and zero_pad is not None:
            zero_pad_rows(out, *zero_pad)
        return out
    if out is None:
        shape = (batch, M, N) if batch > 1 else (M, N)
        out = torch.empty(shape, dtype=out_dtype, device=A.device)       # split-K: the entry zeroes C itself
        ldc = N
        sC = M * N
    out_f32 = 1 if out.dtype == torch.float32 else 0
    call("ds2_gemm_nt_coresident" if coresident else "ds2_gemm_nt", dt(A), P(A), P(B), P(out), PF(bias), M, N, K, lda, ldb, ldc,
         out_f32, batch, sA, sB, sC, sBias, splitk, S())
    if rows is not None and zero_pad is not None and batch == 1:
        zero_pad_rows(out, *zero_pad)          # same contract whichever kernel ran: unlisted rows are zero
    return out


def kslice_plan(K, slices):
    """(slices, Ks): how a contraction of length K is cut for gemm_nt_kslices -- the wanted slice count or the next smaller one (down
    to half) that divides the 64-element tiles, slices of Ks = whole tiles each (+ a rest of K - slices * Ks).  The one place that
    decides it: fc_bwd cuts its rows the same way, which is what keeps its dW bit for bit the K-sliced product's."""
    nkt = K // 64
    for s_ in range(slices, max(1, slices // 2), -1):   # a slice count that divides the 64-element tiles leaves no rest
        if nkt % s_ == 0 and K % 64 == 0:
            slices = s_
            break
    return slices, (K // max(slices, 1)) // 64 * 64


def head_kslices(R):
    """K-slices of the output layer's weight gradient over R rows (model._HeadFn, both of its paths)."""
    return max(1, min(32, R // 2048))


def gemm_nt_kslices(A, B, slices):
    """C[M][N] f32 = A[M][K] * B[N][K]^T (2-D row-major A, B) with the contraction cut into `slices` K-slices of equal length (whole
    64-element tiles) that run as the kernel's BATCH into a [slices (+1 for the rest of K)][M][N] scratch and are added in index order
    (ds2_sum_slices): split-K with a fixed summation order, so the result is the same in every run (atomic split-K is not)."""
    M, K = A.shape[-2], A.shape[-1]
    N = B.shape[-2]
    lda, ldb = A.stride(-2), B.stride(-2)
    slices, Ks = kslice_plan(K, slices)
    if slices <= 1 or Ks == 0 or (M * N) % 4 != 0:
        return gemm_nt(A, B, out_dtype=torch.float32)
    rest = K - slices * Ks
    ws = torch.empty((slices + (1 if rest else 0), M, N), dtype=torch.float32, device=A.device)
    call("ds2_gemm_nt", dt(A), P(A), P(B), P(ws), None, M, N, Ks, lda, ldb, N, 1, slices, Ks, Ks, M * N, 0, 1, S())
    if rest:
        call("ds2_gemm_nt", dt(A), P(A[:, slices * Ks:]), P(B[:, slices * Ks:]), P(ws[slices]), None, M, N, rest, lda, ldb, N, 1, 1,
             0, 0, 0, 0, 1, S())
    out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    call("ds2_sum_slices", P(ws), P(out), M * N, ws.shape[0], S())
    return out


FC_CALLS = {"fwd": 0, "bwd": 0}     # launches of the output-layer kernels (tests assert that the model routes through them)


def fc_ok(dtype, H, Cp):
    """Shapes the output-layer kernels take: bf16 activations, 32 or 64 padded classes, H % 8 == 0 and a weight that fits their LDS."""
    return dtype == torch.bfloat16 and bool(query("ds2_fc_supported", int(H), int(Cp)))


def fc_fwd(Xh, Wp, R=None, H=None):
    """logits [R][Cp] f32 = Xh[R][H] * Wp[Cp][H]^T (bf16 operands; Xh may carry a padded row stride) -- one pass over Xh."""
    R = Xh.shape[0] if R is None else R
    H = Wp.shape[1] if H is None else H
    Cp = Wp.shape[0]
    logits = torch.empty((R, Cp), dtype=torch.float32, device=Xh.device)
    call("ds2_fc_fwd", P(Xh), Xh.stride(0), P(Wp), Wp.stride(0), P(logits), Cp, R, H, Cp, S())
    FC_CALLS["fwd"] += 1
    return logits


def fc_bwd(dlogits, Xh, Wp, R=None, H=None):
    """(dXh [R][H] bf16 = bf16(dlogits) * Wp, dW [Cp][H] f32 = bf16(dlogits)^T * Xh) from dlogits and Xh as stored: no cast pass, no
    transposes.  dW's row blocks are the K-slices gemm_nt_kslices would cut (kslice_plan) and are added in index order (no atomics);
    both results have the bits of gemm_nt(bf16(dlogits), Wp^T) and gemm_nt_kslices(dlogits^T, Xh^T, head_kslices(R))."""
    R = Xh.shape[0] if R is None else R
    H = Wp.shape[1] if H is None else H
    Cp = Wp.shape[0]
    dev = Xh.device
    K = rup(R, 64)                       # the transposed operands' contraction length (ops.transpose pads the rows to whole tiles)
    slices, Ks = kslice_plan(K, head_kslices(R))
    block_rows = K if slices <= 1 or Ks == 0 else Ks
    dXh = torch.empty((R, H), dtype=torch.bfloat16, device=dev)
    dW = torch.empty((Cp, H), dtype=torch.float32, device=dev)
    ws = torch.empty((query("ds2_fc_bwd_partials", R, block_rows), Cp, H), dtype=torch.float32, device=dev)
    call("ds2_fc_bwd", PF(dlogits), dlogits.stride(0), P(Xh), Xh.stride(0), P(Wp), Wp.stride(0), P(dXh), H, P(dW), P(ws), R, H, Cp,
         block_rows, S())
    FC_CALLS["bwd"] += 1
    return dXh, dW


FP32_KSPLIT = __import__("os").environ.get("DS2_FP32_KSPLIT", "1") != "0"    # 0: every exact-fp32 product in one pass (round 5)


def fp32_ksplit(dtype, M, N, K):
    """K-slices of an exact-fp32 product (ops.gemm_nt): > 1 when its 128x128 tiles fill less than half of the chip and the
    contraction is long; a divisor of the K-tile count (32 elements) so that every slice is whole tiles of the same length."""
    if not FP32_KSPLIT or dtype != torch.float32 or K % 32 != 0 or (M * N) % 4 != 0:
        return 1
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    nkt = K // 32
    if tiles >= 128 or nkt < 32:
        return 1
    want = min(8, max(1, 256 // tiles))
    for s_ in range(want, 1, -1):
        if nkt % s_ == 0 and nkt // s_ >= 8:
            return s_
    return 1


def gemm_nt_rows2(A, A2, m_split, B, M, N, K, lda, ldb, splitk=1, coresident=False):
    """C[M][N] f32 = [A rows 0..m_split-1 ; A2 rows 0..M-m_split-1][.][K] * B[N][K]^T: the A operand split over two buffers."""
    out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    call("ds2_gemm_nt_rows2", dt(A), P(A), P(A2), m_split, P(B), P(out), M, N, K, lda, ldb, N, 1, splitk, 1 if coresident else 0, S())
    return out


def gemm8_nt(A, B, bias=None, out_dtype=None, M=None, N=None, K=None, lda=None, ldb=None, rows=None, stagger_us=None, out=None):
    """C[M][N] = A[M][K] * B[N][K]^T (+bias) on the 256x256 phase-split kernel (bf16 operands, K % 64 == 0); rows: see gemm_nt.
    stagger_us (tests, A/B): the span of the first round's start offsets in microseconds, clamped to
    query("ds2_gemm8_stagger_plan", -1, 0, 0); None = the library's policy.  The result does not depend on it.
    out: write into this [M][>= N] tensor (bf16 or fp32, unit column stride; its row stride is C's leading dimension) instead of a
    new one -- a column window of a wider buffer; with `rows` the unlisted rows keep what they held."""
    M = A.shape[-2] if M is None else M
    N = B.shape[-2] if N is None else N
    K = A.shape[-1] if K is None else K
    lda = A.stride(-2) if lda is None else lda
    ldb = B.stride(-2) if ldb is None else ldb
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype or A.dtype, device=A.device)
    elif out.dim() != 2 or out.shape[0] < M or out.shape[1] < N or out.stride(1) != 1 or out.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("gemm8_nt: out must be a [>= %d][>= %d] bf16 / fp32 tensor with unit column stride" % (M, N))
    ldc = out.stride(0)
    if stagger_us is not None:
        call("ds2_gemm8_nt_rows_stagger", P(A), P(B), P(out), PF(bias), M, N, K, lda, ldb, ldc, 1 if out.dtype == torch.float32 else 0, P(rows),
             rows.numel() if rows is not None else 0, int(stagger_us), S())
        return out
    if rows is not None:
        call("ds2_gemm8_nt_rows", P(A), P(B), P(out), PF(bias), M, N, K, lda, ldb, ldc, 1 if out.dtype == torch.float32 else 0, P(rows),
             rows.numel(), S())
        return out
    call("ds2_gemm8_nt", P(A), P(B), P(out), PF(bias), M, N, K, lda, ldb, ldc, 1 if out.dtype == torch.float32 else 0, S())
    return out


def gemm8_tn_grouped(problems, K, dx=None, rows=None, zero_pad=None):
    """problems: list of dicts(At, Bt, M, N, lda, ldb[, At2, lda2, m_split][, out]); every product C[M][N] f32 = sum_{k<K} At[k][m] Bt[k][n]
    in one launch.  Returns the list of outputs.  dx = (A, B): additionally the NT product A[M][Kx] * B[N][Kx]^T (bf16) in the SAME
    launch (the layer's dX beside its weight gradients); returns (outputs, dX) then.  rows: the contraction (and the rows of dX)
    runs over the listed rows only; zero_pad = (lens, Tp, N) zeroes the unlisted rows of dX."""
    rp, nr = (P(rows), rows.numel()) if rows is not None else (None, 0)
    n = len(problems)
    outs = []
    for pr in problems:
        o = pr.get("out")
        if o is None:
            o = torch.empty((pr["M"], pr["N"]), dtype=torch.float32, device=pr["At"].device)
        outs.append(o)
    vp = C.c_void_p * n
    ia, la = C.c_int * n, C.c_long * n
    At = vp(*[pr["At"].data_ptr() for pr in problems])
    At2 = vp(*[(pr["At2"].data_ptr() if pr.get("At2") is not None else 0) for pr in problems])
    ms = ia(*[int(pr.get("m_split", 0)) for pr in problems])
    Bt = vp(*[pr["Bt"].data_ptr() for pr in problems])
    Cs = vp(*[o.data_ptr() for o in outs])
    Ms, Ns = ia(*[pr["M"] for pr in problems]), ia(*[pr["N"] for pr in problems])
    lda, ldb = la(*[pr["lda"] for pr in problems]), la(*[pr["ldb"] for pr in problems])
    lda2 = la(*[int(pr.get("lda2", 0)) for pr in problems])
    ldc = la(*[o.stride(0) for o in outs])
    for pr in problems:
        P(pr["At"]), P(pr["Bt"])            # refuses CPU tensors
    if dx is not None:
        A, B = dx
        Mx, Nx, Kx = A.shape[0], B.shape[0], A.shape[1]
        out_x = torch.empty((Mx, Nx), dtype=A.dtype, device=A.device)
        call("ds2_gemm8_wgrad_dx_rows", n, At, At2, ms, Bt, Cs, Ms, Ns, lda, lda2, ldb, ldc, K, P(A), P(B), P(out_x), Mx, Nx, Kx, A.stride(0),
             B.stride(0), Nx, rp, nr, S())
        if rows is not None and zero_pad is not None:
            zero_pad_rows(out_x, *zero_pad)
        return outs, out_x
    call("ds2_gemm8_tn_grouped_rows", n, At, At2, ms, Bt, Cs, Ms, Ns, lda, lda2, ldb, ldc, K, rp, nr, S())
    return outs


def colsum(X, R=None, Cc=None, ld=None, scale=1.0):
    R = X.shape[0] if R is None else R
    Cc = X.shape[1] if Cc is None else Cc
    ld = X.stride(0) if ld is None else ld
    out = torch.empty(Cc, dtype=torch.float32, device=X.device)
    ws = torch.empty(query("ds2_norm_partials", R) * Cc, dtype=torch.float32, device=X.device)
    call("ds2_colsum", dt(X), P(X), R, Cc, ld, P(out), float(scale), P(ws), S())
    return out


# fp32 (1e-3 parity) mode: a large GEMM can run as ONE bf16 GEMM over three K-segments of split operands (a_hi b_hi + a_hi b_lo +
# a_lo b_hi, fp32 accumulation: ~2e-5 of |a||b| per entry against 6e-8 of the exact-fp32 MFMA, which runs at 1/16 of the bf16 rate).
# Default ("wgrad"): only the WEIGHT-GRADIENT products, whose results are leaves -- 2e-5 stays 2e-5.  The input projections and dX
# feed the recurrence / the layers below, and a deep stack amplifies their noise: with every GEMM split the conv1 weight gradient of
# the 7-layer LSTM-1280 fixture lands 3.8e-3 from the reference (bar 1e-3), although logits and loss stay inside 1e-3
# (DS2_FP32_GEMM=split3: config 2 10.8 ms instead of 12.3; =exact: no split anywhere).
import os as _os
FP32_GEMM_MODE = _os.environ.get("DS2_FP32_GEMM", "wgrad")
FP32_SPLIT3 = FP32_GEMM_MODE != "exact"


def split3_ok(dtype, M, N, K, leaf=False):
    """leaf: the product is a parameter gradient (its error does not propagate)."""
    if dtype != torch.float32 or FP32_GEMM_MODE == "exact" or not (M >= 256 and N >= 256 and K >= 256):
        return False
    return leaf or FP32_GEMM_MODE == "split3"


def split3(X, mode, out=None):
    """fp32 [rows][K] (any row stride) -> bf16 [rows][3 * Kp], Kp = K rounded up to 64: K-segments [hi | hi | lo] (mode 0: the A
    operand of a product) or [hi | lo | hi] (mode 1: the B operand).  `out`: a row window of a larger [.., 3 * Kp] buffer."""
    rows, K = X.shape
    Kp = rup(K, 64)
    if out is None:
        out = torch.empty((rows, 3 * Kp), dtype=torch.bfloat16, device=X.device)
    assert out.shape[0] == rows and out.shape[1] == 3 * Kp and X.dtype == torch.float32 and X.stride(1) == 1
    call("ds2_split3_bf16", P(X), X.stride(0), rows, K, Kp, mode, P(out), out.stride(0), S())
    return out


def split3_rows(X, mode):
    """fp32 [rows][K] (any row stride) -> bf16 [3 * rows][K8] (K8 = K rounded up to 8, zero beyond K): the split segments stacked by
    rows, [hi; hi; lo] (mode 0: the At operand of a TN product) or [hi; lo; hi] (mode 1: the Bt operand).  The contraction of
    ds2_gemm8_tn_grouped over the 3 * rows rows of two such operands = a_hi b_hi + a_hi b_lo + a_lo b_hi."""
    rows, K = X.shape
    K8 = rup(K, 8)
    out = torch.empty((3 * rows, K8), dtype=torch.bfloat16, device=X.device)
    assert X.dtype == torch.float32 and X.stride(1) == 1
    call("ds2_split3_bf16", P(X), X.stride(0), rows, K, K8, 2 + mode, P(out), K8, S())
    return out


def transpose(X, R=None, Cc=None, lds=None):
    """dst[C][ldd] = X[R][C]^T with ldd = roundup(R, 64) (the K-tile of the MFMA GEMM) and zero fill of the pad columns."""
    R = X.shape[0] if R is None else R
    Cc = X.shape[1] if Cc is None else Cc
    lds = X.stride(0) if lds is None else lds
    ldd = rup(R, 64)
    out = torch.empty((Cc, ldd), dtype=X.dtype, device=X.device)
    call("ds2_transpose", dt(X), P(X), P(out), R, Cc, lds, ldd, S())
    return out


def cast_transpose_bf16(src, dst=None, ldd=0, dstT=None, lddT=0, perm=None, cout=None):
    """fp32 parameter matrix -> bf16 copy (window `dst`, row stride ldd) and/or bf16 transpose (window `dstT`, row stride
    lddT); `perm` = (c, f) re-orders the conv features of rnns.0, `cout` pads the columns with zeros."""
    R, Cc = src.shape
    pc, pf = perm if perm is not None else (0, 0)
    call("ds2_cast_transpose_bf16", PF(src), src.stride(0), R, Cc, pc, pf, Cc if cout is None else cout,
         P(dst) if dst is not None else None, ldd, P(dstT) if dstT is not None else None, lddT, S())


def small_weight_layouts(w1, w2, wfc, dtype):
    """(w1k, w2t, [w2d_even, w2d_odd], wfc_padded, wfcT) in kernel layout from the fp32 parameters -- one launch."""
    dev, Cc, H = w1.device, wfc.shape[0], wfc.shape[1]
    w1k = torch.empty((451, 32), dtype=torch.float32, device=dev)
    w2t = torch.empty((21, 11, 32, 32), dtype=dtype, device=dev)
    w2d0 = torch.empty((11, 11, 32, 32), dtype=dtype, device=dev)
    w2d1 = torch.empty((10, 11, 32, 32), dtype=dtype, device=dev)
    wp = torch.empty((32, H), dtype=dtype, device=dev)
    wpT = torch.empty((H, 32), dtype=dtype, device=dev)
    call("ds2_small_weight_layouts", dt(dtype), PF(w1), PF(w2), PF(wfc), Cc, H, P(w1k), P(w2t), P(w2d0), P(w2d1), P(wp), P(wpT), S())
    return w1k, w2t, [w2d0, w2d1], wp, wpT


def scale_by_(x, s):
    """x *= s[0] in place (x f32 contiguous, s a device scalar tensor)."""
    call("ds2_scale_by", P(x), PF(s.reshape(1)), x.numel(), S())
    return x


def add2(a, b):
    out = torch.empty_like(a)
    call("ds2_add2", dt(a), P(a), P(b), P(out), a.numel(), S())
    return out


class BnSaved:
    __slots__ = ("mean", "rstd", "scale", "shift")

    def __init__(self, Cc, device):
        buf = torch.empty((4, Cc), dtype=torch.float32, device=device)
        self.mean, self.rstd, self.scale, self.shift = buf[0], buf[1], buf[2], buf[3]


def bn_fwd(X, mode, training, gamma, beta, rmean, rvar, nbt, R, Cc, ldx, Y, ldy, F=0, Tp=0, N=0, lens=None, eps=1e-5,
           momentum=0.1):
    sv = BnSaved(Cc, X.device)
    ws = torch.empty(2 * query("ds2_norm_partials", R) * Cc, dtype=torch.float32, device=X.device)
    call("ds2_bn_fwd", dt(X), mode, 1 if training else 0, P(X), P(Y), R, Cc, ldx, ldy, F, Tp, N, P(lens), PF(gamma), PF(beta),
         PF(rmean), PF(rvar), P(nbt) if training else C.c_void_p(0), float(eps), float(momentum), P(sv.mean), P(sv.rstd),
         P(sv.scale), P(sv.shift), P(ws), S())
    return sv


def bn_bwd(G, X, DX, mode, sv, R, Cc, ldg, ldx, lddx, F=0, Tp=0, N=0, lens=None):
    dgamma = torch.empty(Cc, dtype=torch.float32, device=X.device)
    dbeta = torch.empty(Cc, dtype=torch.float32, device=X.device)
    ws = torch.empty((2 * query("ds2_norm_partials", R) + 2) * Cc, dtype=torch.float32, device=X.device)
    call("ds2_bn_bwd", dt(X), mode, P(G), P(X), P(DX), R, Cc, ldg, ldx, lddx, F, Tp, N, P(lens), P(sv.mean), P(sv.rstd),
         P(sv.scale), P(sv.shift), P(dgamma), P(dbeta), P(ws), S())
    return dgamma, dbeta


# ---------------------------------------------------------------------------------------------------------------
def conv_rows(F0):
    """(F1, F2): frequency rows after conv1 / conv2 for F0 input bins (reference model.py:166-168): 161 -> (81, 41), 81 -> (41, 21)."""
    F1 = (F0 + 2 * 20 - 41) // 2 + 1
    return F1, (F1 + 2 * 10 - 21) // 2 + 1


def conv1_fwd(x, w1k, b1, lens, Tp, dtype):
    N, _, F0, T = x.shape
    y1 = torch.empty((N, conv_rows(F0)[0], Tp, 32), dtype=dtype, device=x.device)
    call("ds2_conv1_fwd", dt(dtype), PF(x), PF(w1k), PF(b1), P(lens), P(y1), N, F0, T, Tp, S())
    return y1


def conv1_wgrad(x, dy1, Tp):
    N, _, F0, T = x.shape
    dw = torch.empty((451, 32), dtype=torch.float32, device=x.device)
    ws = torch.empty(query("ds2_conv1_wgrad_ws_floats", N, F0, Tp), dtype=torch.float32, device=x.device)
    call("ds2_conv1_wgrad", dt(dy1), P(x), P(dy1), P(dw), N, F0, T, Tp, P(ws), S())
    return dw


def conv2_fwd(a1, w2t, b2, lens, F0=161):
    N, F1, Tp, _ = a1.shape
    assert F1 == conv_rows(F0)[0]
    y2 = torch.empty((N, conv_rows(F0)[1], Tp, 32), dtype=a1.dtype, device=a1.device)
    nws = query("ds2_conv2_fwd_ws_bytes", dt(a1), N, F0, Tp)
    ws = torch.empty(nws, dtype=torch.uint8, device=a1.device) if nws else None
    call("ds2_conv2_fwd", dt(a1), P(a1), P(w2t), PF(b2), P(lens), P(y2), N, F0, Tp, P(ws), S())
    return y2


def conv2_dgrad(dy2, w2d_even, w2d_odd, F0=161):
    N, F2, Tp, _ = dy2.shape
    assert F2 == conv_rows(F0)[1]
    da1 = torch.empty((N, conv_rows(F0)[0], Tp, 32), dtype=dy2.dtype, device=dy2.device)
    call("ds2_conv2_dgrad", dt(dy2), P(dy2), P(w2d_even), P(w2d_odd), P(da1), N, F0, Tp, S())
    return da1


def conv2_wgrad(dy2, a1, F0=161):
    N, _, Tp, _ = dy2.shape
    dw = torch.empty((231, 32, 32), dtype=torch.float32, device=dy2.device)
    ws = torch.empty(query("ds2_conv2_wgrad_ws_floats", N, Tp), dtype=torch.float32, device=dy2.device)
    call("ds2_conv2_wgrad", dt(dy2), P(dy2), P(a1), P(dw), N, F0, Tp, P(ws), S())
    return dw


# ---------------------------------------------------------------------------------------------------------------
_PERSIST_ERR = {}
LAST_PERSIST_WS = None   # the most recent persistent sweep's scratch (its tail holds the kernel's cycle counters)

# ---- per-launch options of the persistent sweeps (ds2_persist_opts) -----------------------------------------------------------
# What the host decides per launch: the routing A/B bits and the fault-injection spin budget (tests / tools only, through the
# persist_options() context, which restores them on exit whatever happens inside), and the START-UP budget -- how long the sweep's
# workgroups wait for all of them to become resident (a sweep needs every CU at once):
#   * single process: 300 ms.  Nothing legitimate holds compute units that long; fail fast, error code 2 names the cause.
#   * data parallel (torch.distributed initialised with > 1 rank, or dist.wrap_data_parallel told model.py): the process group's
#     time-out (torch's default for "nccl": 10 min).  An RCCL all-reduce on DDP's stream stays resident until its SLOWEST peer
#     arrives -- the reference's sampler hands ranks unequal batches (loader/data_loader.py:320-360), rank 0 saves checkpoints,
#     loaders stall -- and a sweep launched behind it must WAIT, exactly as a stock kernel would queue; if a peer is really gone
#     the collective's own watchdog ends the job, not the sweep.
#   * DS2_PERSIST_STARTUP_MS overrides both.
STARTUP_MS_SINGLE = 300
STARTUP_MS_DP_MIN, STARTUP_MS_DP_MAX = 30_000, 3_600_000
_OPTS = {"variant": 0, "spin_limit": 0, "startup_ms": None}
FORCE_DATA_PARALLEL_BUDGET = [False]      # model.PER_LAYER_NODES_FOR_DDP's twin: dist.wrap_data_parallel sets it for DS2_FORCE_DDP runs


class persist_options:
    """with ops.persist_options(variant=..., spin_limit=..., startup_ms=...): every persistent sweep launched inside (forward on this
    thread, backward on autograd's) carries these ds2_persist_opts; the previous values come back on exit."""

    def __init__(self, **kw):
        assert set(kw) <= set(_OPTS), kw
        self.kw = kw

    def __enter__(self):
        self.old = dict(_OPTS)
        _OPTS.update(self.kw)
        return self

    def __exit__(self, *exc):
        _OPTS.clear()
        _OPTS.update(self.old)
        return False


def data_parallel_ranks():
    """World size of the initialised default process group (1 if none)."""
    try:
        import torch.distributed as _dist
        if _dist.is_available() and _dist.is_initialized():
            return int(_dist.get_world_size())
    except Exception:  # noqa: BLE001
        pass
    return 1


def persist_startup_ms():
    """The start-up budget the next sweep is launched with (see above)."""
    if _OPTS["startup_ms"] is not None:
        return int(_OPTS["startup_ms"])
    env = _os.environ.get("DS2_PERSIST_STARTUP_MS", "")
    if env:
        return max(1, int(env))
    if data_parallel_ranks() > 1 or FORCE_DATA_PARALLEL_BUDGET[0]:
        ms = 600_000
        try:
            import torch.distributed as _dist
            from torch.distributed.distributed_c10d import _get_default_group
            if _dist.is_initialized():
                to = getattr(_get_default_group(), "_timeout", None) or getattr(_dist, "default_pg_timeout", None)
                if to is not None:
                    ms = int(to.total_seconds() * 1000)
        except Exception:  # noqa: BLE001
            pass
        return min(max(ms, STARTUP_MS_DP_MIN), STARTUP_MS_DP_MAX)
    return STARTUP_MS_SINGLE


def _persist_opts():
    """(ctypes struct, byref) for one launch; the struct must stay alive until the call returns."""
    o = _lib.PersistOpts(int(_OPTS["variant"]), int(_OPTS["spin_limit"]), persist_startup_ms())
    return o


def persist_kind(dtype, kind, D, N, H):
    """Kernel family the persistent entries run for the problem on the current device under the current routing (0 none, 1 / 2 tuned
    H = 1024, 3 round-4 general, 4 round-2 general)."""
    return query("ds2_rnn_persist_kind", dt(dtype), CELLS[kind], D, N, H, int(_OPTS["variant"]))


def _persist_err(dev):
    """One int32 word per device that the persistent recurrent kernels raise when a workgroup times out."""
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    t = _PERSIST_ERR.get(key)
    if t is None:
        t = _PERSIST_ERR[key] = torch.zeros(16, dtype=torch.int32, device=dev)
    return t


def _persist_error_message(code, key):
    """The sticky error word of the persistent sweeps: 1 = a workgroup gave up waiting for a peer's data in the middle of a sweep,
    2 = the start-up wait never completed, i.e. the sweep's workgroups (one whole CU each) were not all resident."""
    if code == 2:
        return ("a persistent recurrent sweep on device %d could not start: its workgroups never became co-resident within its start-up "
                "budget (%.1f s now; 0.3 s single-process, the process group's time-out under data parallelism, DS2_PERSIST_STARTUP_MS "
                "overrides) -- another kernel holds compute units (a second process on this GPU, e.g. a validation job or two ranks with "
                "the same LOCAL_RANK; or a long-running kernel on another stream).  The sweep gave up, its outputs were NaN-poisoned"
                % (key, persist_startup_ms() / 1000.0))
    return ("a persistent recurrent kernel timed out on device %d waiting for its peer workgroups in the middle of a sweep "
            "(are other kernels occupying CUs?); its outputs were NaN-poisoned" % key)


def check_persistent_kernels():
    """Synchronises and raises if any persistent recurrent kernel launched so far gave up waiting for its peers."""
    for key, t in _PERSIST_ERR.items():
        code = int(t[0].item())
        if code != 0:
            raise _lib.Ds2HipError(_persist_error_message(code, key))


_ERR_MIRROR = {}   # device index -> [pinned host int32 tensor, event of the copy in flight or None]


def poll_persistent_error(dev):
    """Surfaces a timed-out persistent sweep WITHOUT a host synchronisation (DeepSpeech.training_step calls this once per
    step): raises if the asynchronous copy of the device's error word enqueued by an earlier call has landed non-zero,
    then enqueues a fresh copy behind the work queued so far.  A stalled sweep therefore raises one step late at the
    latest; its outputs are NaN-poisoned meanwhile (and the CTC loss stays NaN), never silently zero."""
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    t = _PERSIST_ERR.get(key)
    if t is None:
        return
    m = _ERR_MIRROR.get(key)
    if m is None:
        m = _ERR_MIRROR[key] = [torch.zeros(1, dtype=torch.int32).pin_memory(), None]
    if m[1] is not None:
        if not m[1].query():
            return                                   # the previous copy has not landed yet: look again next step
        m[1] = None
        if int(m[0][0]) != 0:
            raise _lib.Ds2HipError(_persist_error_message(int(m[0][0]), key))
    call("ds2_copy_words", P(t), C.c_void_p(m[0].data_ptr()), 1, S())      # in-stream kernel -> pinned host word (no SDMA transfer)
    ev = torch.cuda.Event()
    ev.record()
    m[1] = ev


class PinnedRing:
    """Host staging for the small per-step int32 tables (lengths + row list, CTC target table): ONE pinned allocation per ring, made at
    first use, cut into `depth` slots that are reused round-robin behind an event each.

    Why not ``torch.empty(..., pin_memory=True)`` per step: torch's pinned-block cache hands a block out again only after the copy
    that read it has finished.  A training loop's host thread runs several steps ahead of the device until the hardware queue is
    full, so during the first second of a run every step allocated FRESH pinned blocks (hipHostMalloc: device page-table edits under
    the running kernels), and the copies themselves went to the SDMA engines, where the transfers of LATER steps run under the
    kernels of earlier ones: a recurrent sweep (latency-bound, all 256 CUs polling L2) hit by one took 2.1-3.0 ms instead of 1.0-1.3
    -- 11 of the first 19 timed steps of a bench run, i.e. most of the window the driver times (tools/step_jitter.py,
    profiles/r05c_step_jitter.txt, r05d_step_jitter_env.txt).  The slot is therefore copied by an in-stream kernel (ds2_copy_words)."""

    def __init__(self, depth=32):
        self.depth = depth
        self._per_device = {}          # device index -> _RingState: slots, events and the copy kernel's stream belong to ONE device
        self._lock = __import__("threading").Lock()

    class _RingState:
        def __init__(self):
            self.cap, self.buf, self.events, self.i = 0, None, None, 0

    def stage(self, dev, parts):
        """parts: 1-D int32 numpy arrays -> their concatenation as ONE int32 device tensor (asynchronous copy on `dev`'s current
        stream; `dev` need not be the current device)."""
        n = int(sum(p.size for p in parts))
        dev = torch.device(dev)
        if dev.type != "cuda":
            return torch.from_numpy(np.concatenate([np.asarray(p, dtype=np.int32).reshape(-1) for p in parts]) if parts else np.zeros(0, np.int32))
        key = dev.index if dev.index is not None else torch.cuda.current_device()
        with self._lock, torch.cuda.device(key):
            st = self._per_device.setdefault(key, PinnedRing._RingState())
            if st.buf is None or n > st.cap:
                if st.events is not None:
                    for e in st.events:               # the old buffer must outlive the copies that still read it
                        if e is not None:
                            e.synchronize()
                st.cap = max(1024, 1 << (max(n, 1) - 1).bit_length())
                st.buf = torch.empty(self.depth * st.cap, dtype=torch.int32, pin_memory=True)
                st.events = [None] * self.depth
                st.i = 0
            k = st.i
            st.i = (k + 1) % self.depth
            if st.events[k] is not None and not st.events[k].query():
                st.events[k].synchronize()            # the host is a whole ring ahead of the device: wait for the slot's last copy
            slot = st.buf[k * st.cap:k * st.cap + n]
            hv = slot.numpy()
            o = 0
            for p in parts:
                hv[o:o + p.size] = np.asarray(p).reshape(-1)
                o += p.size
            out = torch.empty(n, dtype=torch.int32, device=torch.device("cuda", key))
            if n:
                # a kernel that reads the (device-mapped) pinned slot, not hipMemcpyAsync: see ds2_copy_words for what SDMA transfers
                # of later steps cost the sweeps of earlier ones.  The kernel needs the slot's DEVICE address: equal to the host
                # address for torch's default pinned allocator (hipHostMalloc, unified addressing); with
                # PYTORCH_CUDA_ALLOC_CONF=pinned_use_cuda_host_register the two can differ, and the copy goes through torch instead
                dptr = _pinned_device_ptr(slot)
                if dptr is not None:
                    call("ds2_copy_words", C.c_void_p(dptr), P(out), n, S())
                else:
                    out.copy_(slot, non_blocking=True)
            if st.events[k] is None:
                st.events[k] = torch.cuda.Event()
            st.events[k].record()
            return out


_HIPRT = []


def _pinned_device_ptr(t):
    """Device address of a pinned host tensor (hipHostGetDevicePointer), or None if the runtime cannot give one."""
    if not _HIPRT:
        try:
            lib = C.CDLL("libamdhip64.so")
            lib.hipHostGetDevicePointer.restype = C.c_int
            lib.hipHostGetDevicePointer.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint]
            _HIPRT.append(lib)
        except OSError:
            _HIPRT.append(None)
    lib = _HIPRT[0]
    if lib is None:
        return t.data_ptr()                           # no runtime library to ask: unified addressing is the default
    dp = C.c_void_p(0)
    rc = lib.hipHostGetDevicePointer(C.byref(dp), C.c_void_p(t.data_ptr()), 0)
    return dp.value if rc == 0 and dp.value else None


POISON_UNWRITTEN = False  # tests: the BPTT outputs start as NaN, so a consumer that reads a row the sweep was allowed to leave
                          # unwritten (rnn_bwd(pad_rows_unread=True)) shows up as NaN gradients
PERSIST_ENABLED = True   # tests flip this to run the per-time-step kernels on shapes the persistent kernels cover


_WARNED_CUS = set()
_WARNED_SHAPES = set()
PERSIST_CLIFF_MIN_H = 256      # below this width a time step is launch-bound either way: no warning


def use_persistent(kind, dtype, D, N, H):
    """True if a persistent sweep (one launch per layer and direction pair) takes this problem on the current device.  Never a
    silent cliff: when the answer is no because the DEVICE exposes fewer than 256 CUs although the shape is covered (partition /
    CU-mask modes) that is an error unless DS2_ALLOW_LAUNCH_PER_STEP=1 -- a CU-masked rank of a data-parallel job must not quietly
    become the straggler; when no persistent kernel is instantiated for the shape (the reference leaves hidden_size free,
    train_config.py:49) the launch-per-time-step kernels run, 5-8x slower per step, and a warning says so once per shape."""
    if not PERSIST_ENABLED:
        return False
    ok = bool(query("ds2_rnn_persist_supported", dt(dtype), CELLS[kind], D, N, H, int(_OPTS["variant"])))
    if ok:
        return True
    import os
    import warnings
    covered = bool(query("ds2_rnn_persist_shape_covered", dt(dtype), CELLS[kind], D, N, H))
    if covered:
        dev = torch.cuda.current_device()
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        if os.environ.get("DS2_ALLOW_LAUNCH_PER_STEP", "0") in ("", "0"):
            raise _lib.Ds2HipError("ds2hip: device %d exposes %d compute units (< 256): the persistent recurrent kernels need one "
                                   "workgroup per CU, all co-resident.  Set DS2_ALLOW_LAUNCH_PER_STEP=1 to run the launch-per-time-step "
                                   "kernels instead (several times slower)." % (dev, cus))
        if dev not in _WARNED_CUS:
            _WARNED_CUS.add(dev)
            warnings.warn("ds2hip: device %d exposes %d compute units (< 256): the persistent recurrent kernels are disabled, the "
                          "recurrent sweeps use one launch per time step" % (dev, cus))
    elif H >= PERSIST_CLIFF_MIN_H:
        key = (kind, str(dtype), D, N, H)
        if key not in _WARNED_SHAPES:
            _WARNED_SHAPES.add(key)
            # the widths a full device takes for this dtype, cell, direction count and batch (csrc/ds2_rnn_persist_widths.h is the list)
            widths = [w for w in range(16, 2049, 16) if query("ds2_rnn_persist_shape_covered", dt(dtype), CELLS[kind], D, N, w)]
            warnings.warn("ds2hip: no persistent recurrent kernel is instantiated for %s %s hidden=%d, %d direction(s), batch %d: the "
                          "sweeps run one launch per time step (5-8x slower per step).  For this cell, type, direction count and batch "
                          "persistent kernels exist with hidden in {%s}; the model class zero-pads other hidden sizes up to the nearest "
                          "instantiated width when that is at most 1.5x as wide (DS2_PAD_HIDDEN)."
                          % (str(dtype).replace("torch.", ""), kind, H, D, N, ", ".join(map(str, widths))))
    return False


def rnn_fwd(kind, GI, Whh, bhh, lens, D, N, H, Tp, h0=None, c0=None, save=True):
    """Returns (HseqExt [D][Tp+2][N][H] with zero guard slots, S, hn [D,N,H] f32, cn or None)."""
    dev, dtype = GI.device, GI.dtype
    hext = torch.empty((D, Tp + 2, N, H), dtype=dtype, device=dev)
    persistent = use_persistent(kind, dtype, D, N, H)
    if not persistent:                    # the persistent kernels zero the guard slots themselves
        hext[:, 0].zero_()
        hext[:, Tp + 1].zero_()
    ns = SAVED_PLANES[kind]
    Sv = torch.empty((D, Tp, N, max(ns, 1) * H) if ns else (1,), dtype=dtype, device=dev)
    hn = torch.empty((D, N, H), dtype=torch.float32, device=dev)
    cn = torch.empty((D, N, H), dtype=torch.float32, device=dev) if kind == "lstm" else None
    if persistent:
        ws = torch.empty(query("ds2_rnn_persist_ws_bytes", dt(dtype), CELLS[kind], D, N, H, int(_OPTS["variant"])), dtype=torch.uint8, device=dev)
        global LAST_PERSIST_WS
        LAST_PERSIST_WS = ws
        po = _persist_opts()
        with _sweep_timer("rnn_fwd_persistent", Tp):
            call("ds2_rnn_persist_fwd", dt(dtype), CELLS[kind], D, N, H, Tp, P(lens), P(GI), P(Whh), PF(bhh), PF(h0), PF(c0),
                 P(hext[:, 1]), (Tp + 2) * N * H, P(Sv), P(hn), P(cn), P(ws), P(_persist_err(dev)), C.byref(po), S())
        return hext, Sv, hn, cn
    state = torch.empty(query("ds2_rnn_state_bytes", D, N, H), dtype=torch.uint8, device=dev)
    with _sweep_timer("rnn_fwd", Tp):
        call("ds2_rnn_fwd", dt(dtype), CELLS[kind], D, N, H, Tp, P(lens), P(GI), P(Whh), PF(bhh), PF(h0), PF(c0),
             P(hext[:, 1]), (Tp + 2) * N * H, P(Sv), P(hn), P(cn), P(state), S())
    return hext, Sv, hn, cn


class RnnGrads:
    """What a BPTT sweep hands to the weight-gradient stage.  dGI [Tp*N][D*G*H]: gradient of the input projection (= of the
    hidden-side pre-activations too, except the GRU's n slot).  GRU only: either dGH [D][Tp][N][3H] (per-time-step kernels: the
    full hidden-side gradient [dr, dz, dQ]) or dQ [D][Tp][N][H] (persistent kernels: only the slot that differs from dGI).
    bacc [D][N][NB*H] f32 or None: per-sample sums over time of the gate-gradient planes (persistent kernels)."""
    __slots__ = ("dGI", "dGH", "dQ", "bacc", "dh0", "dc0")

    def __init__(self, dGI, dGH=None, dQ=None, bacc=None):
        self.dGI, self.dGH, self.dQ, self.bacc = dGI, dGH, dQ, bacc
        self.dh0 = self.dc0 = None          # d loss / d initial state (rnn_bwd(want_dstate=True))

    def tensors(self):
        return [t for t in (self.dGI, self.dGH, self.dQ, self.bacc) if t is not None]


def rnn_bwd(kind, dOut, WhhT, hext, Sv, lens, D, N, H, Tp, pad_rows_unread=False, h0=None, c0=None, want_dstate=False):
    """pad_rows_unread: the caller reads dGI / dQ only through a row list of the real frames (and takes the bias gradients from the
    sweep's per-sample sums): a persistent sweep that leaves the padding rows unwritten then does not zero them.
    h0 / c0 [D][N][H] f32: the initial state the forward was given (reference model.py:224-230); want_dstate: also return d loss /
    d h0 (and d c0) as RnnGrads.dh0 / .dc0.  Either routes the sweep to the launch-per-time-step BPTT (the persistent sweeps assume a
    zero initial state in backward; training through a given `hs` is the rare path)."""
    dev, dtype = dOut.device, dOut.dtype
    G = GATES[kind]
    dGI = torch.empty((Tp * N, D * G * H), dtype=dtype, device=dev)
    with_state = h0 is not None or c0 is not None or want_dstate
    if not with_state and use_persistent(kind, dtype, D, N, H):
        dQ = torch.empty((D, Tp, N, H), dtype=dtype, device=dev) if kind == "gru" else None
        if POISON_UNWRITTEN:
            dGI.fill_(float("nan"))
            if dQ is not None:
                dQ.fill_(float("nan"))
        bacc = torch.empty((D, N, (4 if kind == "gru" else G) * H), dtype=torch.float32, device=dev)
        ws = torch.empty(query("ds2_rnn_persist_ws_bytes", dt(dtype), CELLS[kind], D, N, H, int(_OPTS["variant"])), dtype=torch.uint8, device=dev)
        global LAST_PERSIST_WS
        LAST_PERSIST_WS = ws
        po = _persist_opts()
        with _sweep_timer("rnn_bwd_persistent", Tp):
            call("ds2_rnn_persist_bwd", dt(dtype), CELLS[kind], D, N, H, Tp, P(lens), P(dOut), P(WhhT), P(hext[:, 1]), (Tp + 2) * N * H,
                 P(Sv), P(dGI), P(dQ), P(bacc), 1 if pad_rows_unread else 0, P(ws), P(_persist_err(dev)), C.byref(po), S())
        return RnnGrads(dGI, dQ=dQ, bacc=bacc)
    dGH = torch.empty((D, Tp, N, G * H), dtype=dtype, device=dev) if kind == "gru" else None
    state = torch.empty(query("ds2_rnn_state_bytes", D, N, H), dtype=torch.uint8, device=dev)
    dh0 = torch.empty((D, N, H), dtype=torch.float32, device=dev) if want_dstate else None
    dc0 = torch.empty((D, N, H), dtype=torch.float32, device=dev) if (want_dstate and kind == "lstm") else None
    with _sweep_timer("rnn_bwd", Tp):
        call("ds2_rnn_bwd", dt(dtype), CELLS[kind], D, N, H, Tp, P(lens), P(dOut), P(WhhT), P(hext[:, 1]), (Tp + 2) * N * H,
             P(Sv), P(dGI), P(dGH), PF(h0), PF(c0), P(dh0), P(dc0), P(state), S())
    rg = RnnGrads(dGI, dGH=dGH)
    rg.dh0, rg.dc0 = dh0, dc0
    return rg


# ---------------------------------------------------------------------------------------------------------------
def rnn_bias_grads(kind, bacc, D, N, H):
    """(bias_ih.grad [D*G*H], bias_hh.grad [D][G*H]) from the BPTT sweep's per-sample sums bacc [D][N][NB*H] -- one launch."""
    G = GATES[kind]
    dbih = torch.empty(D * G * H, dtype=torch.float32, device=bacc.device)
    dbhh = torch.empty((D, G * H), dtype=torch.float32, device=bacc.device)
    call("ds2_rnn_bias_grads", CELLS[kind], D, N, H, PF(bacc), P(dbih), P(dbhh), S())
    return dbih, dbhh


def lookahead_fwd(x, w, Tp, N, H, save=True):
    y = torch.empty_like(x)
    pre = torch.empty_like(x) if save else None
    call("ds2_lookahead_fwd", dt(x), P(x), PF(w), P(y), P(pre), Tp, N, H, w.shape[1], S())
    return y, pre


def lookahead_bwd(x, w, pre, dy, Tp, N, H):
    ctx = w.shape[1]
    dx = torch.empty_like(x)
    dw = torch.empty((H, ctx), dtype=torch.float32, device=x.device)
    ws = torch.empty(query("ds2_lookahead_ws_floats", Tp, N, H, ctx), dtype=torch.float32, device=x.device)
    call("ds2_lookahead_bwd", dt(x), P(x), P(w), P(pre), P(dy), P(dx), P(dw), Tp, N, H, ctx, P(ws), S())
    return dx, dw


def softmax_rows(logits, Cc):
    rows = logits.shape[0]
    out = torch.empty((rows, Cc), dtype=torch.float32, device=logits.device)
    call("ds2_softmax_rows", P(logits), P(out), rows, Cc, logits.stride(0), Cc, S())
    return out


def greedy_decode(scores, sizes, blank, _words=None):
    """scores: (N, T', C) f32 CUDA tensor (any strides with a contiguous class dimension); sizes: [N] int tensor.
    Returns host lists (tokens per sample, frame offsets per sample) -- reference decoder.py:164-181."""
    scores = _f32_classes(scores)
    N, T, Cc = scores.shape
    dev = scores.device
    sz = sizes.to(dev, torch.int32) if sizes is not None else None
    buf = torch.empty((2, N, T), dtype=torch.int32, device=dev)
    counts = torch.empty(N, dtype=torch.int32, device=dev)
    call("ds2_greedy_decode", P(scores), scores.stride(0), scores.stride(1), N, T, Cc, P(sz), blank, P(buf[0]), P(buf[1]), P(counts),
         S())
    if _words is not None:       # decode_words: the confidence pass reads the device buffers before anything travels
        return _words_to_host(scores, sz, buf[0][:, None], buf[1][:, None], counts[:, None], blank, _words, _words["kind"])
    return _greedy_to_host(buf, counts)


def _greedy_to_host(buf, counts):
    """host lists (labels per sample, their frames per sample) from a greedy decode's buf (2, N, T) and counts [N]"""
    N = counts.shape[0]
    cnt = counts.cpu()
    width = int(cnt.max().item()) if N > 0 else 0
    host = buf[:, :, :max(width, 1)].cpu()           # only the surviving labels + offsets travel
    toks = [host[0, i, :int(cnt[i])].tolist() for i in range(N)]
    offs = [host[1, i, :int(cnt[i])] for i in range(N)]
    return toks, offs


BEAM_MAX_WIDTH, BEAM_MAX_TOP_N, BEAM_MAX_CLASSES = 256, 64, 8192     # ds2_beam_decode's limits


BEAM_LM_MAX_ORDER = 5


def beam_search(probs, sizes, blank, beam_width, cutoff_top_n, cutoff_prob, lm=None, hot=None, _words=None):
    """CTC prefix beam search (ds2_beam_decode and its _lm, _hot and _lm_hot forms): the one body of beam_decode, beam_decode_lm,
    beam_decode_hot and beam_decode_lm_hot.  probs: (N, T', C) CUDA tensor of probabilities (any strides with a contiguous class
    dimension); sizes: [N] int tensor or None (= T').  lm, hot: None, or the dicts that beam_stream_open takes (lm with
    unit="char": a character model, ds2_beam_decode_clm, which takes no hot words).  Returns host
    lists: tokens[n][b] (labels of beam b, best first), offsets[n][b] (int tensor of their frames), a host (N, B) float tensor of
    scores (-log p less the LM's and the hot words' terms: the total that ranked the beams; +inf where fewer than B beams are
    alive) and one of the acoustic -log p of the same beams, which with neither an LM nor hot words is scores.  Only the
    surviving labels, their frames and the scores travel."""
    N, T, Cc = probs.shape
    B, top_n, lm, hot = _beam_settings(Cc, probs.device, beam_width, cutoff_top_n, blank, lm, hot)
    if N == 0 or T == 0:
        return _beam_no_frames(N, B)
    probs = _f32_classes(probs)
    dev = probs.device
    sz = sizes.to(dev, torch.int32) if sizes is not None else None
    buf, lens, scores = _beam_outputs(N, B, T, dev)
    ws = torch.empty(query("ds2_beam_ws_bytes", N, T, B), dtype=torch.uint8, device=dev)
    _beam_launch(probs, sz, blank, B, top_n, cutoff_prob, lm, hot, buf, lens, scores, ws)
    plain = lm is None and hot is None
    if _words is not None:
        sc = scores[:1 if plain else 2].cpu()
        return _words_to_host(probs, sz, buf[0], buf[1], lens, blank, _words) + (sc[0], sc[-1])
    return _beam_to_host(buf, lens, scores, N, B, plain=plain)


def beam_search_device(probs, sizes, blank, beam_width, cutoff_top_n, cutoff_prob, lm=None, hot=None):
    """beam_search without the trip to the host: the same checks and the same launch, and the tensors of _beam_outputs come back as
    they are -- buf (2, N, B, T') int32 = tokens and offsets, lens (N, B) int32, scores (2, N, B) f32 = ranking and acoustic (the
    plain form leaves the second plane unwritten; a rank with no beam alive has score +inf).  probs needs frames (N, T' > 0)."""
    N, T, Cc = probs.shape
    B, top_n, lm, hot = _beam_settings(Cc, probs.device, beam_width, cutoff_top_n, blank, lm, hot)
    if N == 0 or T == 0:
        raise ValueError("beam_search_device needs at least one clip and one frame, got probs of shape %s" % (tuple(probs.shape),))
    if not probs.is_cuda:
        raise ValueError("beam_search_device needs a HIP device tensor; there is no CPU fallback")
    probs = _f32_classes(probs)
    dev = probs.device
    sz = sizes.to(dev, torch.int32) if sizes is not None else None
    buf, lens, scores = _beam_outputs(N, B, T, dev)
    ws = torch.empty(query("ds2_beam_ws_bytes", N, T, B), dtype=torch.uint8, device=dev)
    _beam_launch(probs, sz, blank, B, top_n, cutoff_prob, lm, hot, buf, lens, scores, ws)
    return buf, lens, scores


def beam_decode(probs, sizes, blank, beam_width, cutoff_top_n, cutoff_prob, _words=None):
    """CTC prefix beam search without a language model (ds2_beam_decode).  probs: (N, T', C) CUDA tensor of probabilities (any
    strides with a contiguous class dimension); sizes: [N] int tensor or None (= T').  Returns host lists: tokens[n][b] (labels
    of beam b, best first), offsets[n][b] (int tensor of their frames) and a host (N, B) float tensor of scores (-log p, ctcdecode's
    convention; +inf where fewer than B beams are alive).  Only the surviving labels, their frames and the scores travel."""
    res = beam_search(probs, sizes, blank, beam_width, cutoff_top_n, cutoff_prob, _words=_words)
    return res if len(res) == 5 else res[:3]         # five: the values of the _words pass, which end in scores and acoustic


def beam_decode_lm(probs, sizes, blank, beam_width, cutoff_top_n, cutoff_prob, space, word_table, ngram_table, order, bos,
                   alpha, beta, lexicon=True, _words=None):
    """CTC prefix beam search with a word n-gram language model (ds2_beam_decode_lm).  Arguments as beam_decode, plus the space
    label, the two tables of lm.build_tables as int64 CUDA tensors of shape (slots, 2) on the device of probs, the LM's order,
    the id of <s>, alpha, beta and the lexicon flag.  Returns beam_decode's three values, scores being -(log p + lm), and a host
    (N, B) float tensor of the acoustic -log p of the same beams."""
    lm = dict(space=space, word_table=word_table, ngram_table=ngram_table, order=order, bos=bos, alpha=alpha, beta=beta,
              lexicon=lexicon)
    return beam_search(probs, sizes, blank, beam_width, cutoff_top_n, cutoff_prob, lm, _words=_words)


def beam_decode_clm(probs, sizes, blank, beam_width, cutoff_top_n, cutoff_prob, label_ids, ngram_table, order, bos, alpha, beta,
                    _words=None):
    """CTC prefix beam search with a character n-gram language model (ds2_beam_decode_clm): every label is an event of the
    model.  Arguments as beam_decode, plus the two values of lm.build_char_tables on the device of probs (label_ids: int32 [C],
    the unigram id of every class, -1 for none, the blank's entry ignored; ngram_table: int64 (slots, 2)), the LM's order, the id
    of <s>, alpha and beta.  Returns beam_decode_lm's four values; there is no end-of-utterance term."""
    lm = dict(unit="char", label_ids=label_ids, ngram_table=ngram_table, order=order, bos=bos, alpha=alpha, beta=beta)
    return beam_search(probs, sizes, blank, beam_width, cutoff_top_n, cutoff_prob, lm, _words=_words)


def beam_decode_hot(probs, sizes, blank, beam_width, cutoff_top_n, cutoff_prob, space, hot_table, _words=None):
    """beam_decode with hot words (ds2_beam_decode_hot).  space: the space label; hot_table: the table of hotwords.build_table
    as an int64 CUDA tensor of shape (slots, 2) on the device of probs.  Returns beam_decode's three values, scores being
    -(log p + hot_end), the total that ranked the beams, and a host (N, B) float tensor of the acoustic -log p of the same beams."""
    return beam_search(probs, sizes, blank, beam_width, cutoff_top_n, cutoff_prob, None, dict(space=space, table=hot_table),
                       _words=_words)


def beam_decode_lm_hot(probs, sizes, blank, beam_width, cutoff_top_n, cutoff_prob, space, word_table, ngram_table, order, bos,
                       alpha, beta, lexicon, hot_table, hot_oov_logp, _words=None):
    """beam_decode_lm with hot words (ds2_beam_decode_lm_hot): its arguments, the table of hotwords.build_table and the ln P that a
    covered out-of-vocabulary word event is charged.  Returns beam_decode_lm's four values, scores being -((log p + lm) + hot_end)."""
    lm = dict(space=space, word_table=word_table, ngram_table=ngram_table, order=order, bos=bos, alpha=alpha, beta=beta,
              lexicon=lexicon)
    return beam_search(probs, sizes, blank, beam_width, cutoff_top_n, cutoff_prob, lm,
                       dict(space=space, table=hot_table, oov_logp=hot_oov_logp), _words=_words)


def _f32_classes(x):
    """x (N, T, C) as the decode kernels read it: float32 with a contiguous class dimension; copies only where it has to"""
    if x.dtype != torch.float32:
        x = x.float()
    if x.stride(2) != 1:
        x = x.contiguous()
    return x


def _space_check(Cc, blank, space):
    if not 0 <= space < Cc or space == blank:
        raise ValueError("space label %d must be one of the %d classes and differ from the blank (%d)" % (space, Cc, blank))


def _table_check(name, t, device):
    """The checks of an open-addressing table (word_table, ngram_table, hot_table) for a search on `device`."""
    if not (torch.is_tensor(t) and t.dtype == torch.int64 and t.dim() == 2 and t.shape[1] == 2 and t.is_contiguous()):
        raise ValueError("%s must be a contiguous int64 tensor of shape (slots, 2)" % name)
    if t.shape[0] < 2 or t.shape[0] & (t.shape[0] - 1):
        raise ValueError("%s: the number of slots must be a power of two >= 2, got %d" % (name, t.shape[0]))
    if t.device != device or not t.is_cuda:
        raise ValueError("%s must live on the device of the probabilities (%s), not %s" % (name, device, t.device))


def _hot_checks(Cc, device, blank, space, hot_table, hot_oov_logp=0.0):
    """The argument checks of the hot-word calls: the space label, the table of hotwords.build_table on `device`, hot_oov_logp."""
    _space_check(Cc, blank, space)
    _table_check("hot_table", hot_table, device)
    v = float(hot_oov_logp)
    if v != v or v in (float("inf"), float("-inf")) or abs(v) > 3.4e38:
        raise ValueError("hot_oov_logp must be a finite fp32 value, got %r" % (hot_oov_logp,))


def _beam_lm_checks(Cc, device, beam_width, cutoff_top_n, blank, space, word_table, ngram_table, order, bos):
    """The argument checks of a search with a language model, for Cc classes on `device`, which is all that they look at of the
    probabilities (beam_stream_open has none); returns (B, top_n)."""
    B, top_n = _beam_checks(Cc, beam_width, cutoff_top_n, blank)
    _space_check(Cc, blank, space)
    if not 1 <= int(order) <= BEAM_LM_MAX_ORDER:
        raise ValueError("language-model order must be in [1, %d], got %d" % (BEAM_LM_MAX_ORDER, order))
    if bos < 0:
        raise ValueError("the id of <s> must not be negative, got %d" % bos)
    _table_check("word_table", word_table, device)
    _table_check("ngram_table", ngram_table, device)
    return B, top_n


def _lm_is_char(lm):
    """whether the lm dict of a search names a character language model (unit="char"; absent or "word": a word model)"""
    if lm is None:
        return False
    unit = lm.get("unit", "word")
    if unit not in ("word", "char"):
        raise ValueError("the language model's unit must be 'word' or 'char', got %r" % (unit,))
    return unit == "char"


def _beam_clm_checks(Cc, device, beam_width, cutoff_top_n, blank, label_ids, ngram_table, order, bos):
    """The argument checks of a search with a character language model, in the manner of _beam_lm_checks; returns (B, top_n)."""
    B, top_n = _beam_checks(Cc, beam_width, cutoff_top_n, blank)
    if not 1 <= int(order) <= BEAM_LM_MAX_ORDER:
        raise ValueError("language-model order must be in [1, %d], got %d" % (BEAM_LM_MAX_ORDER, order))
    if bos < 0:
        raise ValueError("the id of <s> must not be negative, got %d" % bos)
    if not (torch.is_tensor(label_ids) and label_ids.dtype == torch.int32 and label_ids.dim() == 1 and label_ids.shape[0] == Cc
            and label_ids.is_contiguous()):
        raise ValueError("label_ids must be a contiguous int32 tensor with one entry per class (%d)" % Cc)
    if label_ids.device != device or not label_ids.is_cuda:
        raise ValueError("label_ids must live on the device of the probabilities (%s), not %s" % (device, label_ids.device))
    _table_check("ngram_table", ngram_table, device)
    return B, top_n


def _beam_settings(Cc, device, beam_width, cutoff_top_n, blank, lm, hot):
    """The argument checks of beam_search and beam_stream_open, in their order: the search's own, the language model's, the hot
    words'.  Returns (B, top_n, lm, hot), the dicts with every scalar as the C call takes it."""
    if lm is None:
        B, top_n = _beam_checks(Cc, beam_width, cutoff_top_n, blank)
    elif _lm_is_char(lm):
        if hot is not None:
            raise ValueError("hot words are defined on word boundaries; a character language model takes none")
        B, top_n = _beam_clm_checks(Cc, device, beam_width, cutoff_top_n, blank, lm["label_ids"], lm["ngram_table"], lm["order"],
                                    lm["bos"])
        lm = dict(unit="char", label_ids=lm["label_ids"], ngram_table=lm["ngram_table"], order=int(lm["order"]),
                  bos=int(lm["bos"]), alpha=float(lm["alpha"]), beta=float(lm["beta"]))
    else:
        B, top_n = _beam_lm_checks(Cc, device, beam_width, cutoff_top_n, blank, lm["space"], lm["word_table"], lm["ngram_table"],
                                   lm["order"], lm["bos"])
        lm = dict(lm, space=int(lm["space"]), order=int(lm["order"]), bos=int(lm["bos"]), alpha=float(lm["alpha"]),
                  beta=float(lm["beta"]), lexicon=bool(lm.get("lexicon", True)))
    if hot is not None:
        _hot_checks(Cc, device, blank, int(hot["space"]), hot["table"], hot.get("oov_logp", 0.0))
        hot = dict(space=int(hot["space"]), table=hot["table"], oov_logp=float(hot.get("oov_logp", 0.0)))
        if lm is not None and lm["space"] != hot["space"]:
            raise ValueError("the language model and the hot words must name one space label, got %d and %d"
                             % (lm["space"], hot["space"]))
    return B, top_n, lm, hot


# The C entries of the one-shot and of the resumable search, by (language model, hot words).  After the arguments that all share
# come _lm_block, then _hot_block, then the entry's own state and outputs.
_BEAM_CLM_ENTRIES = ("ds2_beam_decode_clm", "ds2_beam_stream_feed_clm")     # a character LM: its own block, never hot words
_BEAM_ENTRIES = {(False, False): ("ds2_beam_decode", "ds2_beam_stream_feed"),
                 (True, False): ("ds2_beam_decode_lm", "ds2_beam_stream_feed_lm"),
                 (False, True): ("ds2_beam_decode_hot", "ds2_beam_stream_feed_hot"),
                 (True, True): ("ds2_beam_decode_lm_hot", "ds2_beam_stream_feed_lm_hot")}


def _beam_entry(lm, hot, stream):
    """the name of the one-shot (stream = 0) or resumable (1) C entry of a search with these dicts"""
    if _lm_is_char(lm):
        return _BEAM_CLM_ENTRIES[stream]
    return _BEAM_ENTRIES[lm is not None, hot is not None][stream]


def _lm_block(lm):
    """the language model's arguments in the C order: space, word_table, slots, ngram_table, slots, order, bos, alpha, beta, lexicon;
    of a character model: label_ids, ngram_table, slots, order, bos, alpha, beta"""
    if lm is None:
        return ()
    if _lm_is_char(lm):
        gt = lm["ngram_table"]
        return (P(lm["label_ids"]), P(gt), gt.shape[0], lm["order"], lm["bos"], lm["alpha"], lm["beta"])
    wt, gt = lm["word_table"], lm["ngram_table"]
    return (lm["space"], P(wt), wt.shape[0], P(gt), gt.shape[0], lm["order"], lm["bos"], lm["alpha"], lm["beta"], int(lm["lexicon"]))


def _hot_block(lm, hot):
    """the hot words' arguments in the C order: table, slots, oov_logp after a language model's block; space, table, slots alone"""
    if hot is None:
        return ()
    table = (P(hot["table"]), hot["table"].shape[0])
    return (hot["space"],) + table if lm is None else table + (hot["oov_logp"],)


def _beam_launch(probs, sz, blank, B, top_n, cutoff_prob, lm, hot, buf, lens, scores, ws):
    """the launch of beam_search on ready tensors (probs f32 with contiguous classes, the outputs of _beam_outputs, ws of
    ds2_beam_ws_bytes) and checked settings; acoustic, scores[1], exists for every form but the plain one"""
    N, T, Cc = probs.shape
    acoustic = () if lm is None and hot is None else (P(scores[1]),)
    call(_beam_entry(lm, hot, 0), P(probs), probs.stride(0), probs.stride(1), N, T, Cc, P(sz), int(blank),
         B, top_n, float(cutoff_prob), *_lm_block(lm), *_hot_block(lm, hot), P(buf[0]), P(buf[1]), P(lens), P(scores[0]), *acoustic,
         P(ws), S())


def _beam_outputs(N, R, ld, dev):
    """the device outputs of a search that keeps R ranks in rows of ld labels: buf (2, N, R, ld) int32 = tokens and offsets,
    lens (N, R) int32, scores (2, N, R) f32 = ranking and acoustic (the plain form leaves the second plane unwritten)"""
    return (torch.empty((2, N, R, ld), dtype=torch.int32, device=dev), torch.empty((N, R), dtype=torch.int32, device=dev),
            torch.empty((2, N, R), dtype=torch.float32, device=dev))


def _beam_to_host(buf, lens, scores, N, R, cap=None, plain=False):
    """tokens, offsets, scores and acoustic on the host from _beam_outputs' tensors after a launch; cap: the rows' width where
    a length can pass it; plain: there is no acoustic plane, and acoustic is scores"""
    ln = lens.cpu().numpy()
    width = max(int(ln.max()), 1) if cap is None else min(max(int(ln.max()), 1), cap)
    host = buf[:, :, :, :width].cpu().numpy()        # only the surviving labels + offsets travel
    toks = [[host[0, n, b, :ln[n, b]].tolist() for b in range(R)] for n in range(N)]
    offs = [[torch.from_numpy(host[1, n, b, :ln[n, b]]) for b in range(R)] for n in range(N)]
    sc = scores[:1 if plain else 2].cpu()
    return toks, offs, sc[0], sc[-1]


def _beam_no_frames(N, B):
    """no frames: the only beam is the empty string, score 0 (it has earned no boost either)"""
    scores = torch.full((N, B), float("inf"))
    scores[:, 0] = 0.0
    return [[[] for _ in range(B)] for _ in range(N)], \
        [[torch.zeros(0, dtype=torch.int32) for _ in range(B)] for _ in range(N)], scores, scores.clone()


BEAM_GRID_MAX_POINTS = 65535     # points of one ds2_beam_decode_lm_grid launch


def plan_grid_chunks(G, bytes_one, bytes_per_point, max_ws_bytes, max_points=BEAM_GRID_MAX_POINTS):
    """Splits the points 0 .. G-1 of a grid decode into consecutive chunks [(start, count), ...] whose workspace,
    bytes_one + (count - 1) * bytes_per_point, fits max_ws_bytes; as few chunks as that allows, the earlier ones full.
    ValueError when one point alone does not fit."""
    G, bytes_one, bytes_per_point, max_ws_bytes = int(G), int(bytes_one), int(bytes_per_point), int(max_ws_bytes)
    if G < 1:
        raise ValueError("the grid needs at least one point, got %d" % G)
    if bytes_one > max_ws_bytes:
        raise ValueError("max_ws_bytes=%d is below the workspace of a single point (%d bytes)" % (max_ws_bytes, bytes_one))
    per = max_points if bytes_per_point <= 0 else min(max_points, 1 + (max_ws_bytes - bytes_one) // bytes_per_point)
    return [(g, min(per, G - g)) for g in range(0, G, per)]


def _weights(name, w, dev):
    t = torch.as_tensor(w, dtype=torch.float32)
    if t.dim() != 1:
        raise ValueError("%s must be a one-dimensional sequence of floats, got shape %s" % (name, tuple(t.shape)))
    return t.to(dev).contiguous()


def beam_decode_lm_grid(probs, sizes, blank, beam_width, cutoff_top_n, cutoff_prob, space, word_table, ngram_table, order, bos,
                        alphas, betas, lexicon=True, max_ws_bytes=1 << 30):
    """beam_decode_lm at G weight points (alphas[g], betas[g]) in one launch of G x N workgroups (ds2_beam_decode_lm_grid); the
    frames are pruned once.  Returns DEVICE tensors of every point's top beam: tokens [G, N, T'] and offsets [G, N, T'] int32 (the
    first lens[g, n] entries of a row are valid, the rest 0), lens [G, N] int32, scores [G, N] = -(log p + lm) and acoustic [G, N]
    f32; row (g, n) is rank 0 of beam_decode_lm(alpha=alphas[g], beta=betas[g]) bit for bit.  The grid is cut into chunks of
    points whose workspace fits max_ws_bytes (plan_grid_chunks); the cut does not change the result."""
    B, top_n = _beam_lm_checks(probs.shape[2], probs.device, beam_width, cutoff_top_n, blank, space, word_table, ngram_table,
                               order, bos)
    block = (int(space), P(word_table), word_table.shape[0], P(ngram_table), ngram_table.shape[0], int(order), int(bos),
             int(bool(lexicon)))
    return _beam_grid("ds2_beam_decode_lm_grid", probs, sizes, blank, B, top_n, cutoff_prob, block, alphas, betas, max_ws_bytes)


def _beam_grid(entry, probs, sizes, blank, B, top_n, cutoff_prob, block, alphas, betas, max_ws_bytes):
    """the one body of beam_decode_lm_grid and beam_decode_clm_grid after their checks; block: the language model's arguments
    in the C order up to the points"""
    if not probs.is_cuda:
        raise ValueError("probs must be a HIP device tensor")
    N, T, Cc = probs.shape
    dev = probs.device
    al, be = _weights("alphas", alphas, dev), _weights("betas", betas, dev)
    G = al.shape[0]
    if G < 1 or be.shape[0] != G:
        raise ValueError("alphas and betas must have the same length >= 1, got %d and %d" % (G, be.shape[0]))
    buf = torch.zeros((2, G, N, T), dtype=torch.int32, device=dev)
    lens = torch.zeros((G, N), dtype=torch.int32, device=dev)
    scores = torch.zeros((2, G, N), dtype=torch.float32, device=dev)
    if N == 0 or T == 0:             # no frames: the only beam is the empty string, score 0
        return buf[0], buf[1], lens, scores[0], scores[1]
    one = query("ds2_beam_grid_ws_bytes", 1, N, T, B)
    chunks = plan_grid_chunks(G, one, query("ds2_beam_grid_ws_bytes", 2, N, T, B) - one, max_ws_bytes)
    probs = _f32_classes(probs)
    sz = sizes.to(dev, torch.int32) if sizes is not None else None
    ws = torch.empty(query("ds2_beam_grid_ws_bytes", max(c for _, c in chunks), N, T, B), dtype=torch.uint8, device=dev)
    for g0, cnt in chunks:
        g1 = g0 + cnt
        call(entry, P(probs), probs.stride(0), probs.stride(1), N, T, Cc, P(sz), int(blank), B, top_n, float(cutoff_prob), *block,
             cnt, P(al[g0:g1]), P(be[g0:g1]), P(buf[0, g0:g1]), P(buf[1, g0:g1]), P(lens[g0:g1]), P(scores[0, g0:g1]),
             P(scores[1, g0:g1]), P(ws), S())
    return buf[0], buf[1], lens, scores[0], scores[1]


def beam_decode_clm_grid(probs, sizes, blank, beam_width, cutoff_top_n, cutoff_prob, label_ids, ngram_table, order, bos, alphas,
                         betas, max_ws_bytes=1 << 30):
    """beam_decode_clm at G weight points (alphas[g], betas[g]) in one launch of G x N workgroups (ds2_beam_decode_clm_grid), as
    beam_decode_lm_grid: the same DEVICE tensors, row (g, n) being rank 0 of beam_decode_clm(alpha=alphas[g], beta=betas[g]) bit
    for bit."""
    B, top_n = _beam_clm_checks(probs.shape[2], probs.device, beam_width, cutoff_top_n, blank, label_ids, ngram_table, order, bos)
    block = (P(label_ids), P(ngram_table), ngram_table.shape[0], int(order), int(bos))
    return _beam_grid("ds2_beam_decode_clm_grid", probs, sizes, blank, B, top_n, cutoff_prob, block, alphas, betas, max_ws_bytes)


class BeamStreamHandle:
    """The device state of N resumable beam searches (ds2_beam_stream_*): one buffer with every stream's beam state and node pool,
    and the session's settings.  Made by beam_stream_open."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def beam_stream_open(num_streams, max_frames, num_classes, blank, beam_width, cutoff_top_n, cutoff_prob, device="cuda", lm=None,
                     hot=None):
    """Opens N = num_streams resumable CTC prefix beam searches of up to max_frames frames each.  lm: None, or the dict of
    beam_decode_lm's language-model arguments (space, word_table, ngram_table, order, bos, alpha, beta, lexicon), or with
    unit="char" those of beam_decode_clm (label_ids, ngram_table, order, bos, alpha, beta; no hot words then).  hot: None, or
    the dict of the hot-word arguments (space, table, and with an LM oov_logp); the session keeps this table.  The checks and
    messages are beam_decode's / beam_decode_lm's.  The handle owns ds2_beam_stream_bytes(...) bytes of device memory: the
    states and the node pool, 12 * beam_width bytes per frame and stream.  Every stream starts fresh."""
    N, F, Cc = int(num_streams), int(max_frames), int(num_classes)
    dev = torch.device(device)
    if N < 1 or F < 1:
        raise ValueError("a beam stream needs num_streams >= 1 and max_frames >= 1, got %d and %d" % (N, F))
    if dev.type != "cuda":
        raise ValueError("a beam stream lives on a HIP device, not on %s" % dev)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    B, top_n, lm, hot = _beam_settings(Cc, dev, beam_width, cutoff_top_n, blank, lm, hot)
    if (F + 1) * B > 2 ** 31 - 1:
        raise ValueError("max_frames=%d with beam_width=%d passes the node pool's 2^31 - 1 slots per stream" % (F, B))
    # the flag word of the ds2_beam_stream_* size queries: bit 0 an LM, bit 1 hot words, bit 2 the LM scores characters
    flags = int(lm is not None) | (2 if hot is not None else 0) | (4 if _lm_is_char(lm) else 0)
    state = torch.empty(query("ds2_beam_stream_bytes", N, B, F, flags), dtype=torch.uint8, device=dev)
    # state_stride: bytes between two streams' states at the front of the buffer; the node pool follows them
    h = BeamStreamHandle(state=state, N=N, B=B, max_frames=F, C=Cc, blank=int(blank), top_n=top_n, cutoff_prob=float(cutoff_prob),
                         lm=lm, hot=hot, flags=flags, device=dev, state_stride=query("ds2_beam_stream_state_stride", B, flags))
    beam_stream_reset(h)
    return h


def _beam_checks(Cc, beam_width, cutoff_top_n, blank):
    """The argument checks that every beam search shares (beam_decode, _beam_lm_checks, beam_stream_open); returns (B, top_n)."""
    B, top_n = int(beam_width), int(cutoff_top_n)
    if not 1 <= B <= BEAM_MAX_WIDTH:
        raise ValueError("beam_width must be in [1, %d], got %d" % (BEAM_MAX_WIDTH, B))
    if top_n < 1 or min(top_n, Cc) > BEAM_MAX_TOP_N:
        raise ValueError("min(cutoff_top_n, number of classes) must be in [1, %d], got cutoff_top_n=%d with %d classes"
                         % (BEAM_MAX_TOP_N, top_n, Cc))
    if not 1 <= Cc <= BEAM_MAX_CLASSES:
        raise ValueError("the beam decoder supports up to %d classes, got %d" % (BEAM_MAX_CLASSES, Cc))
    if not 0 <= blank < Cc:
        raise ValueError("blank index %d out of range for %d classes" % (blank, Cc))
    return B, top_n


def beam_stream_reset(h, streams=None):
    """Streams `streams` (indices; None = all) start again from the empty beam; the others are untouched."""
    call("ds2_beam_stream_reset", P(h.state), h.N, h.B, h.max_frames, h.flags, P(_stream_mask(streams, h.N, h.device)), S())


def _beam_stream_call(h, probs, Tc, sz, row_stride, top_only=False):
    """one ds2_beam_stream_feed(_lm) call: a chunk (or none, Tc == 0), with the output stage when row_stride is given; the device
    writes, and the call allocates and copies, R = 1 rank with top_only and all B otherwise"""
    R = 1 if top_only else h.B
    buf = lens = scores = None
    if row_stride is not None:
        row_stride = max(int(row_stride), 1)
        buf, lens, scores = _beam_outputs(h.N, R, row_stride, h.device)
    _beam_stream_launch(h, probs, Tc, sz, buf, lens, scores, row_stride, R)
    if buf is None:
        return None
    plain = h.lm is None and h.hot is None
    res = _beam_to_host(buf, lens, scores, h.N, R, row_stride, plain)
    return res[:3] if plain else res


def _beam_stream_launch(h, probs, Tc, sz, buf, lens, scores, row_stride, R):
    """the launches of _beam_stream_call on the caller's output tensors (_beam_outputs(N, R, row_stride, ...)), or without the
    output stage (buf None); nothing is fetched"""
    ws = torch.empty(query("ds2_beam_stream_ws_bytes", h.N, Tc), dtype=torch.uint8, device=h.device) if Tc > 0 else None
    x = (P(probs), probs.stride(0), probs.stride(1)) if Tc > 0 else (P(None), 0, 0)
    out = (P(buf[0]), P(buf[1]), row_stride, R, P(lens), P(scores[0]), P(scores[1])) if buf is not None else \
        (P(None), P(None), 0, 0, P(None), P(None), P(None))
    if h.lm is None and h.hot is None:       # the plain entry has no acoustic output
        out = out[:-1]
    call(_beam_entry(h.lm, h.hot, 1), *x, h.N, Tc, h.C, P(sz), h.blank, h.B, h.top_n, h.cutoff_prob,
         *_lm_block(h.lm), *_hot_block(h.lm, h.hot), P(h.state), h.max_frames, *out, P(ws), S())


def _sizes_to_device(sizes, dev):
    """a feed's sizes as an int32 tensor on dev (None stays None); host values go through pinned memory, so the copy is queued on
    the stream and the host does not wait for it"""
    if sizes is None:
        return None
    sz = torch.as_tensor(sizes)
    if sz.is_cuda:
        return sz.to(dev, torch.int32)
    return sz.to(torch.int32).pin_memory().to(dev, non_blocking=True)


def beam_stream_feed(h, probs, sizes=None, row_stride=None):
    """Feeds one chunk to the streams of h.  probs: (N, Tc, C) CUDA tensor of probabilities (any strides with a contiguous class
    dimension); sizes: [N] ints (tensor or sequence; None = Tc), the frames of the chunk that each stream takes, 0 leaving it as it
    is.  The call does not wait for the device: host sizes travel through pinned memory in a copy queued on the stream,
    and sizes that are already an int32 tensor on the stream's device are used as they are.  A stream that would pass max_frames takes nothing and has its overflow flag set
    (beam_stream_header).  With row_stride (>= the largest consumed count) the same launch runs the output stage and the call
    returns beam_stream_result's value; otherwise None."""
    if not (torch.is_tensor(probs) and probs.dim() == 3 and probs.shape[0] == h.N and probs.shape[2] == h.C):
        raise ValueError("a chunk for this stream has shape (%d, Tc, %d), got %s"
                         % (h.N, h.C, tuple(probs.shape) if torch.is_tensor(probs) else type(probs).__name__))
    Tc = probs.shape[1]
    if Tc == 0:
        return None if row_stride is None else beam_stream_result(h, row_stride)
    probs = _f32_classes(probs)
    sz = _sizes_to_device(sizes, h.device)
    if sz is not None and sz.shape != (h.N,):
        raise ValueError("sizes must have one entry per stream (%d), got shape %s" % (h.N, tuple(sz.shape)))
    return _beam_stream_call(h, probs, Tc, sz, row_stride)


def beam_stream_result(h, row_stride=None, top_only=False):
    """The beams of every stream on the frames consumed so far: beam_decode's three values (with an LM beam_decode_lm's four, the
    end-of-utterance bonus and re-rank included), equal bit for bit to the one-shot call on those frames.  The state is left
    unchanged, so feeding goes on.  row_stride: an upper bound of the consumed counts (default max_frames), which sizes the device
    rows; only the surviving labels travel.  With top_only the device writes rank 0 alone (rows of row_stride ints per stream,
    not per beam) and every returned list has one entry per stream."""
    return _beam_stream_call(h, None, 0, None, h.max_frames if row_stride is None else row_stride, top_only)


def beam_stream_header(h):
    """Host (N, 3) int32 tensor: per stream the frames consumed, the live beams and the overflow flag (waits for the device)."""
    hdr = h.state[:h.state_stride * h.N].view(h.N, h.state_stride)[:, :16].contiguous().view(torch.int32)
    return hdr[:, :3].cpu()


ENDPOINT_REASONS = (None, "silence", "leading", "length", "final")     # the reason codes of ds2_endpoint_feed / _close
ENDPOINT_STATE_WORDS = 8      # int32 per stream: segment start, trailing, spoken, frames consumed, segments finished, 3 reserved


class EndpointHandle:
    """The device state of N endpointers (ds2_endpoint_*) and their rule.  Made by endpoint_open."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def endpoint_rule_checks(blank_threshold, min_trailing, max_leading, max_segment):
    """The checks of the endpointing rule's parameters; returns them as (float, int, int, int)."""
    thr = float(blank_threshold)
    if not 0.0 < thr < 1.0:
        raise ValueError("blank_threshold must lie in (0, 1), got %r" % (blank_threshold,))
    counts = []
    for name, v in (("min_trailing", min_trailing), ("max_leading", max_leading), ("max_segment", max_segment)):
        if int(v) != v or int(v) < 1:
            raise ValueError("%s must be a frame count >= 1, got %r" % (name, v))
        counts.append(int(v))
    return (thr,) + tuple(counts)


def endpoint_open(num_streams, blank, blank_threshold, min_trailing, max_leading, max_segment, device="cuda"):
    """Opens N = num_streams endpointers with one rule; `blank` is the class whose probability says
    silence.  The handle owns ds2_endpoint_state_bytes(N) bytes of device memory.  Every stream starts at frame 0, segment 0."""
    N = int(num_streams)
    dev = torch.device(device)
    if N < 1:
        raise ValueError("an endpointer needs num_streams >= 1, got %d" % N)
    if dev.type != "cuda":
        raise ValueError("an endpointer lives on a HIP device, not on %s" % dev)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if int(blank) < 0:
        raise ValueError("blank index %d must not be negative" % blank)
    thr, mt, ml, ms = endpoint_rule_checks(blank_threshold, min_trailing, max_leading, max_segment)
    state = torch.empty(query("ds2_endpoint_state_bytes", N) // 4, dtype=torch.int32, device=dev).view(N, ENDPOINT_STATE_WORDS)
    h = EndpointHandle(state=state, N=N, blank=int(blank), blank_threshold=thr, min_trailing=mt, max_leading=ml, max_segment=ms,
                       device=dev)
    endpoint_reset(h)
    return h


def _stream_mask(streams, N, dev):
    """a device int32 mask of the stream indices `streams` (None stays None = all)"""
    if streams is None:
        return None
    m = torch.zeros(N, dtype=torch.int32)
    for n in streams:
        if not 0 <= int(n) < N:
            raise ValueError("stream index %d out of range for %d streams" % (int(n), N))
        m[int(n)] = 1
    return m.pin_memory().to(dev, non_blocking=True)


def endpoint_reset(h, streams=None):
    """Streams `streams` (indices; None = all) start again at frame 0 and segment 0; the others are untouched."""
    call("ds2_endpoint_reset", P(h.state), h.N, P(_stream_mask(streams, h.N, h.device)), S())


def endpoint_feed(h, probs, sizes=None):
    """Advances the endpointers of h over one chunk (ds2_endpoint_feed).  probs: (N, Tc, C) CUDA tensor of probabilities with a
    contiguous class dimension; sizes: [N] ints (tensor or sequence; None = Tc), frames at and beyond them are never read.  Per
    stream the state stops at the first endpoint.  Returns three DEVICE int32 tensors and does not wait for them: cut [N] (the
    chunk's frames that belong to the open segment), rest [N] = sizes - cut, events (4, N) = rows (reason, start, end, index), zero
    where no endpoint fell; reason indexes ENDPOINT_REASONS."""
    if not (torch.is_tensor(probs) and probs.dim() == 3 and probs.shape[0] == h.N and probs.shape[1] >= 1
            and probs.shape[2] > h.blank):
        raise ValueError("a chunk for this endpointer has shape (%d, Tc >= 1, C > %d), got %s"
                         % (h.N, h.blank, tuple(probs.shape) if torch.is_tensor(probs) else type(probs).__name__))
    probs = _f32_classes(probs)
    sz = _sizes_to_device(sizes, h.device)
    if sz is not None and sz.shape != (h.N,):
        raise ValueError("sizes must have one entry per stream (%d), got shape %s" % (h.N, tuple(sz.shape)))
    out = torch.empty((6, h.N), dtype=torch.int32, device=h.device)
    call("ds2_endpoint_feed", P(probs), probs.stride(0), probs.stride(1), h.N, probs.shape[1], probs.shape[2], P(sz), h.blank,
         h.blank_threshold, h.min_trailing, h.max_leading, h.max_segment, P(h.state), P(out[0]), P(out[1]), P(out[2:]), S())
    return out[0], out[1], out[2:]


def endpoint_close(h, streams=None):
    """The open segment of streams `streams` (None = all) ends with reason "final" (ds2_endpoint_close); returns the device
    events (4, N) as endpoint_feed does."""
    ev = torch.empty((4, h.N), dtype=torch.int32, device=h.device)
    call("ds2_endpoint_close", P(h.state), h.N, P(_stream_mask(streams, h.N, h.device)), P(ev), S())
    return ev


def endpoint_state(h):
    """Host (N, 5) int32 tensor: per stream the open segment's start, trailing, spoken, the frames consumed and the segments
    finished (waits for the device)."""
    return h.state[:, :5].cpu()


def endpoint_gather(probs, cut, rest):
    """The frames after the cut at the front of a new contiguous (N, Tc, C) chunk: y[n, :rest[n]] = probs[n, cut[n] : cut[n] +
    rest[n]] (ds2_endpoint_gather); cut, rest: device int32 [N].  The other frames of y are uninitialised."""
    N, Tc, Cc = probs.shape
    y = torch.empty((N, Tc, Cc), dtype=torch.float32, device=probs.device)
    call("ds2_endpoint_gather", P(probs), probs.stride(0), probs.stride(1), N, Tc, Cc, P(cut), P(rest), P(y), S())
    return y


class EndpointSink:
    """Where finished segments wait on the device (endpoint_sink_open): the output stage's tensors of one beam feed and the ring."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def endpoint_sink_open(bh, ranks, row_stride, slots):
    """For the beam streams of handle bh: the stage that a feed's output stage writes (`ranks` best beams per stream, rows of
    row_stride labels) and a ring of `slots` finished segments per stream, ds2_endpoint_ring_bytes(...) bytes."""
    N, R, rs, K = bh.N, int(ranks), int(row_stride), int(slots)
    if not 1 <= R <= bh.B:
        raise ValueError("nbest must be in [1, beam_width = %d], got %d" % (bh.B, R))
    if rs < 1 or K < 1:
        raise ValueError("a segment sink needs row_stride >= 1 and slots >= 1, got %d and %d" % (rs, K))
    dev = bh.device
    words = 4 + 3 * R + 2 * R * rs
    ring = torch.empty(query("ds2_endpoint_ring_bytes", N, K, R, rs) // 4, dtype=torch.int32, device=dev).view(N, K, words)
    buf, lens, scores = _beam_outputs(N, R, rs, dev)
    return EndpointSink(N=N, ranks=R, row_stride=rs, slots=K, words=words, ring=ring,
                        pending=torch.zeros(N, dtype=torch.int32, device=dev), buf=buf, lens=lens, scores=scores,
                        acoustic=bh.lm is not None or bh.hot is not None)


def endpoint_beam_feed(eh, bh, sink, probs, sizes=None):
    """One chunk through the endpointers eh and the beam streams bh, at most one endpoint per stream (the caller keeps chunks to
    min(min_trailing, max_leading, max_segment) frames).  Launch sequence, nothing waits for the device: ds2_endpoint_feed;
    the beam feed of the frames up to the cut with the output stage into the sink's stage; ds2_endpoint_commit, which moves the
    ended streams' rows into their ring; ds2_beam_stream_reset with the events' reason row as its mask; and, for chunks of more
    than one frame, ds2_endpoint_gather, ds2_endpoint_feed and the beam feed again on the frames after the cut."""
    probs = _f32_classes(probs)
    cut, rest, ev = endpoint_feed(eh, probs, sizes)
    _beam_stream_launch(bh, probs, probs.shape[1], cut, sink.buf, sink.lens, sink.scores, sink.row_stride, sink.ranks)
    _endpoint_commit(ev, sink)
    call("ds2_beam_stream_reset", P(bh.state), bh.N, bh.B, bh.max_frames, bh.flags, P(ev[0]), S())
    if probs.shape[1] > 1:                       # a chunk of one frame has no frames after a cut
        y = endpoint_gather(probs, cut, rest)
        endpoint_feed(eh, y, rest)               # no second endpoint can fall here: the chunk is too short for two
        _beam_stream_launch(bh, y, y.shape[1], rest, None, None, None, None, 0)


def endpoint_beam_close(eh, bh, sink, streams=None):
    """The open segments of `streams` (None = all) end with reason "final": their beams, with the end-of-utterance terms of the
    output stage, go to the ring and their searches start again.  Nothing waits for the device."""
    ev = endpoint_close(eh, streams)
    _beam_stream_launch(bh, None, 0, None, sink.buf, sink.lens, sink.scores, sink.row_stride, sink.ranks)
    _endpoint_commit(ev, sink)
    call("ds2_beam_stream_reset", P(bh.state), bh.N, bh.B, bh.max_frames, bh.flags, P(ev[0]), S())


def _endpoint_commit(ev, k):
    call("ds2_endpoint_commit", P(ev), P(k.buf[0]), P(k.buf[1]), k.row_stride, k.ranks, P(k.lens), P(k.scores[0]),
         P(k.scores[1]) if k.acoustic else P(None), k.N, P(k.ring), P(k.pending), k.slots, S())


def endpoint_sink_fetch(k):
    """Fetches and empties the ring (waits for the device).  Returns per stream a list of finished segments in the order they
    ended, each a dict: reason (a string of ENDPOINT_REASONS), start, end, index, labels (ranks lists of ints), offsets (ranks
    int32 tensors, frames counted from the segment's start), scores and acoustic (f32 tensors [ranks])."""
    pend = k.pending.cpu().tolist()
    out = [[] for _ in range(k.N)]
    top = max(pend)
    if top == 0:
        return out
    R, rs = k.ranks, k.row_stride
    host = k.ring[:, :min(top, k.slots)].cpu()
    k.pending.zero_()
    for n in range(k.N):
        for s in range(min(pend[n], k.slots)):
            w = host[n, s]
            lens = w[4:4 + R].tolist()
            sc = w[4 + R:4 + 3 * R].view(torch.float32).clone()
            tok, off = w[4 + 3 * R:4 + 3 * R + R * rs].view(R, rs), w[4 + 3 * R + R * rs:].view(R, rs)
            out[n].append(dict(reason=ENDPOINT_REASONS[int(w[0])], start=int(w[1]), end=int(w[2]), index=int(w[3]),
                               labels=[tok[r, :lens[r]].tolist() for r in range(R)],
                               offsets=[off[r, :lens[r]].clone() for r in range(R)], scores=sc[:R], acoustic=sc[R:]))
    return out


def greedy_stream_feed(scores, sizes, blank, carry):
    """greedy_decode on one chunk of N streams (ds2_greedy_stream_feed).  scores: (N, Tc, C) f32 CUDA tensor; sizes: [N] ints or
    None (= Tc); carry: the (N, 2) int32 CUDA tensor that holds the streams' state between the calls, zeros for fresh streams
    (updated in place).  Returns host lists: the labels that this chunk adds per stream and their frames counted from the start
    of the stream; over all feeds they concatenate to greedy_decode's output on the concatenated input."""
    N, T, Cc = scores.shape
    if not (torch.is_tensor(carry) and carry.is_cuda and carry.dtype == torch.int32 and carry.shape == (N, 2)
            and carry.is_contiguous()):
        raise ValueError("carry must be a contiguous (%d, 2) int32 tensor on the device" % N)
    if N == 0 or T == 0:
        return [[] for _ in range(N)], [torch.zeros(0, dtype=torch.int32) for _ in range(N)]
    scores = _f32_classes(scores)
    dev = scores.device
    sz = _sizes_to_device(sizes, dev)
    buf = torch.empty((2, N, T), dtype=torch.int32, device=dev)
    counts = torch.empty(N, dtype=torch.int32, device=dev)
    call("ds2_greedy_stream_feed", P(scores), scores.stride(0), scores.stride(1), N, T, Cc, P(sz), blank, P(carry), P(buf[0]),
         P(buf[1]), P(counts), S())
    return _greedy_to_host(buf, counts)


ERROR_COUNTS_MAX_LEN = 4096      # ds2_error_counts: labels of one hypothesis or reference


def error_counts(hyp, hyp_lens, targets, target_sizes, space):
    """Character and word error counts on the device (ds2_error_counts), with the semantics of decoder.CharErrorRate /
    WordErrorRate.  hyp: (..., L) int32 CUDA tensor of label rows (P rows in all), hyp_lens: (...) their lengths; targets: the flat
    concatenation of the R references' labels, target_sizes: [R] their lengths, on the host or on the device.  Row p is compared
    with reference p % R.  Returns four device int32 tensors: char_err [P], word_err [P], ref_chars [R], ref_words [R].
    ValueError when a string is longer than ERROR_COUNTS_MAX_LEN labels (one scalar is read back for lengths that live on the
    device and are not bounded by the shapes)."""
    if not (torch.is_tensor(hyp) and hyp.is_cuda and hyp.dim() >= 1):
        raise ValueError("hyp must be a HIP device tensor of label rows")
    dev = hyp.device
    L = hyp.shape[-1]
    hyp = hyp.to(torch.int32).reshape(-1, L).contiguous()
    P_ = hyp.shape[0]
    hl = torch.as_tensor(hyp_lens).to(dev, torch.int32).reshape(-1).contiguous()
    if hl.shape[0] != P_:
        raise ValueError("hyp_lens has %d entries for %d hypotheses" % (hl.shape[0], P_))
    ts = torch.as_tensor(target_sizes).reshape(-1)
    R = ts.shape[0]
    if R < 1 or P_ < R or P_ % R:
        raise ValueError("the number of hypotheses (%d) must be a positive multiple of the number of references (%d)" % (P_, R))
    longest_ref = int(ts.max()) if R else 0               # a scalar read when target_sizes lives on the device
    if longest_ref > ERROR_COUNTS_MAX_LEN or int(ts.min()) < 0:
        raise ValueError("a reference has %d labels; error_counts takes 0 to %d" % (longest_ref, ERROR_COUNTS_MAX_LEN))
    if L > ERROR_COUNTS_MAX_LEN:                           # otherwise the row width bounds every hypothesis
        longest = int(hl.max())
        if longest > ERROR_COUNTS_MAX_LEN:
            raise ValueError("a hypothesis has %d labels; error_counts takes up to %d" % (longest, ERROR_COUNTS_MAX_LEN))
    tg = torch.as_tensor(targets).to(dev, torch.int32).reshape(-1).contiguous()
    offs = torch.zeros(R + 1, dtype=torch.int32, device=dev)
    offs[1:] = torch.cumsum(ts.to(dev, torch.int64), 0)
    if int(ts.sum()) > tg.shape[0]:
        raise ValueError("target_sizes add up to %d labels, targets has %d" % (int(ts.sum()), tg.shape[0]))
    out = torch.empty(2 * P_ + 2 * R, dtype=torch.int32, device=dev)
    ce, we, rc, rw = out[:P_], out[P_:2 * P_], out[2 * P_:2 * P_ + R], out[2 * P_ + R:]
    call("ds2_error_counts", P(hyp), L, P(hl), P_, P(tg), P(offs), R, int(space), P(ce), P(we), P(rc), P(rw), S())
    return ce, we, rc, rw


SPEC_AUGMENT_MAX_MASKS = 4       # ds2_spec_augment / ds2_spectrogram_aug: masks per axis and clip


def _aug_batch(x, frames):
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.shape[1] == 1 and x.dtype == torch.float32):
        raise ValueError("spec_augment takes a float32 HIP device batch of shape (N, 1, F, Tmax)")
    fr = torch.as_tensor(frames).to(x.device, torch.int32).reshape(-1).contiguous()
    if fr.shape[0] != x.shape[0]:
        raise ValueError("frames has %d entries for %d clips" % (fr.shape[0], x.shape[0]))
    return x.contiguous(), fr


def aug_masks(m, N, dev, what):
    """(N, M, 2) int32 device tensor of [start, width] pairs (None = no masks) -> (tensor or None, M)."""
    if m is None:
        return None, 0
    m = torch.as_tensor(m)
    if m.dim() != 3 or m.shape[0] != N or m.shape[2] != 2:
        raise ValueError("%s must have shape (N, masks, 2) = [start, width] per mask; got %s" % (what, tuple(m.shape)))
    if m.shape[1] > SPEC_AUGMENT_MAX_MASKS:
        raise ValueError("%s holds %d masks per clip; the kernels take up to %d" % (what, m.shape[1], SPEC_AUGMENT_MAX_MASKS))
    if m.shape[1] == 0:
        return None, 0
    return m.to(dev, torch.int32).contiguous(), m.shape[1]


def spec_augment_coef(x, frames, warp_draw, W=5):
    """Flow coefficients [N][3] (a_f, a_t, a_0) of the reference's time warp for the clips of x (N, 1, F, Tmax) from the draws
    warp_draw [N][12] (SpecAugment.draw): ds2_spec_augment_coef."""
    x, fr = _aug_batch(x, frames)
    N, _, F, Tmax = x.shape
    wd = torch.as_tensor(warp_draw).to(x.device, torch.float32).contiguous()
    if tuple(wd.shape) != (N, 12):
        raise ValueError("warp_draw must have shape (N, 12); got %s" % (tuple(wd.shape),))
    coef = torch.empty((N, 3), dtype=torch.float32, device=x.device)
    call("ds2_spec_augment_coef", P(x), N, F, Tmax, P(fr), P(wd), int(W), P(coef), S())
    return coef


def spec_augment(x, frames, coef, fmask, tmask):
    """The reference's spec_augment (time warp with the flow coefficients coef [N][3], all zero = none; frequency masks fmask and
    time masks tmask, (N, M, 2) [start, width], None = none) on every clip of the batch x (N, 1, F, Tmax), clip n = its first
    frames[n] frames.  Returns a new tensor; frames beyond a clip's own are zero.  ds2_spec_augment."""
    x, fr = _aug_batch(x, frames)
    N, _, F, Tmax = x.shape
    coef = torch.as_tensor(coef).to(x.device, torch.float32).contiguous()
    if tuple(coef.shape) != (N, 3):
        raise ValueError("coef must have shape (N, 3); got %s" % (tuple(coef.shape),))
    fm, MF = aug_masks(fmask, N, x.device, "fmask")
    tm, MT = aug_masks(tmask, N, x.device, "tmask")
    out = torch.empty_like(x)
    call("ds2_spec_augment", P(x), P(out), N, F, Tmax, P(fr), P(coef), P(fm), MF, P(tm), MT, S())
    return out


CTC_RECURSION = 0    # tests / A-B tools: 0 = pair tiles (default), 1 = always the four-wave recursion kernel, 2 = the one-wave kernel up to 255 labels, 3 = rounds 3-5


def ctc_loss_grad(logits, targets_i32, target_offsets, input_lengths, target_lengths, Tp, N, Cc, blank, max_target_len,
                  ldg=None, recursion=None):
    """logits [Tp*N][ld] f32.  Returns (loss_sum [1], nll [N], dlogits [Tp*N][ldg] f32 with unit upstream gradient)."""
    dev = logits.device
    ldg = logits.shape[1] if ldg is None else ldg
    nll = torch.empty(N, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dlogits = torch.empty((Tp * N, ldg), dtype=torch.float32, device=dev)
    ws = torch.empty(query("ds2_ctc_ws_floats", Tp, N, Cc, max_target_len), dtype=torch.float32, device=dev)
    call("ds2_ctc_loss_grad", P(logits), logits.stride(0), P(targets_i32), P(target_offsets), P(input_lengths),
         P(target_lengths), Tp, N, Cc, blank, max_target_len, 1.0, P(nll), P(loss), P(dlogits), ldg, P(ws),
         int(CTC_RECURSION if recursion is None else recursion), S())
    return loss, nll, dlogits


class CtcMultiState:
    """what ctc_multi_forward(want_grad=True) keeps for ctc_multi_backward: the label rows, the shapes and the workspace"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _ctc_multi_rows(logits, rows, row_lens, input_lengths, Tp, N, Cc, blank):
    """the argument checks of ctc_multi_forward; returns (rows [R][N][ld] int32, lens [R*N] int32, offsets [R*N], input lengths)"""
    if not (torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2
            and logits.stride(1) == 1):
        raise ValueError("logits must be a float32 HIP device tensor [Tp*N][ld] with contiguous classes")
    if Tp < 1 or N < 1 or logits.shape[0] != Tp * N or not 0 < Cc <= logits.shape[1]:
        raise ValueError("logits has shape %s for Tp = %d, N = %d, %d classes" % (tuple(logits.shape), Tp, N, Cc))
    if not 0 <= int(blank) < Cc:
        raise ValueError("blank must be a label in [0, %d), got %r" % (Cc, blank))
    if not (torch.is_tensor(rows) and rows.is_cuda and rows.dim() == 3 and rows.shape[1] == N and rows.shape[0] >= 1):
        raise ValueError("rows must be a HIP device tensor of label rows [R][N][ld] with N = %d" % N)
    dev = logits.device
    R, _, ld = rows.shape
    rows = rows.to(torch.int32).contiguous()
    if ld == 0:                                             # empty rows only: the kernels still take a valid pointer
        rows = torch.zeros((R, N, 1), dtype=torch.int32, device=dev)
    lens = torch.as_tensor(row_lens).to(dev, torch.int32).reshape(-1).contiguous()
    if lens.shape[0] != R * N:
        raise ValueError("row_lens has %d entries for %d x %d rows" % (lens.shape[0], R, N))
    il = torch.as_tensor(input_lengths).to(dev, torch.int32).reshape(-1).contiguous()
    if il.shape[0] != N:
        raise ValueError("input_lengths has %d entries for %d clips" % (il.shape[0], N))
    offs = torch.arange(R * N, dtype=torch.int32, device=dev) * rows.shape[2]
    return rows, lens, offs, il


def ctc_multi_forward(logits, rows, row_lens, input_lengths, Tp, N, Cc, blank, want_grad=False, max_target_len=None,
                      recursion=None):
    """Exact CTC -log p(y | x) of several label rows per clip against the same frames (ds2_ctc_multi_forward): one log-softmax
    per clip, one alpha (and, with want_grad, beta) recursion per row.  logits [Tp*N][ld] f32 (row = t*N + n); rows [R][N][ld]
    int device tensor of labels, row_lens [R][N] their lengths (negative = the row is absent), rank-major as ds2_error_counts
    takes them; input_lengths [N].  max_target_len: the longest row, where the caller knows it (it sizes the workspace; default
    the rows' width).  Returns (nll [R][N] f32: +inf for absent and infeasible rows and clips without frames, state): state is
    None without want_grad, else what ctc_multi_backward takes."""
    rows, lens, offs, il = _ctc_multi_rows(logits, rows, row_lens, input_lengths, Tp, N, Cc, blank)
    dev = logits.device
    R, ld = rows.shape[0], rows.shape[2]
    mtl = ld if max_target_len is None else int(max_target_len)
    if not 0 <= mtl <= ld:
        raise ValueError("max_target_len must be in [0, %d], got %r" % (ld, max_target_len))
    rec = int(CTC_RECURSION if recursion is None else recursion)
    if rec not in (0, 1):
        raise ValueError("ctc_multi_forward runs recursion 0 (pair tiles) or 1 (four waves), got %r" % (rec,))
    nws = query("ds2_ctc_multi_ws_floats", Tp, N, R, Cc, mtl, int(bool(want_grad)))
    if nws < 0:
        raise ValueError("ds2_ctc_multi_forward refuses Tp = %d, N = %d, R = %d, %d classes, %d labels" % (Tp, N, R, Cc, mtl))
    ws = torch.empty(nws, dtype=torch.float32, device=dev)
    nll = torch.empty((R, N), dtype=torch.float32, device=dev)
    call("ds2_ctc_multi_forward", P(logits), logits.stride(0), P(rows), P(offs), P(lens), P(il), Tp, N, R, Cc, int(blank), mtl,
         int(bool(want_grad)), P(nll), P(ws), rec, S())
    if not want_grad:
        return nll, None
    return nll, CtcMultiState(rows=rows, offs=offs, lens=lens, il=il, Tp=Tp, N=N, R=R, Cc=Cc, blank=int(blank), mtl=mtl, ws=ws)


def ctc_multi_backward(state, weights, ldg):
    """dlogits [Tp*N][ldg] f32 = per clip, the sum over its rows in rank order of weights[r][n] * d nll / d logits, log-softmax
    backward fused (ds2_ctc_multi_backward).  state: ctc_multi_forward(want_grad=True)'s; weights [R][N] f32 on the device.  Rows
    whose nll is +inf add nothing whatever their weight; every row and column of dlogits is written."""
    if not isinstance(state, CtcMultiState):
        raise ValueError("state must come from ctc_multi_forward(want_grad=True)")
    s = state
    if not (torch.is_tensor(weights) and weights.is_cuda and weights.dtype == torch.float32 and weights.numel() == s.R * s.N):
        raise ValueError("weights must be a float32 HIP device tensor of %d x %d entries" % (s.R, s.N))
    if int(ldg) < s.Cc:
        raise ValueError("ldg = %r is narrower than the %d classes" % (ldg, s.Cc))
    w = weights.contiguous()
    dlogits = torch.empty((s.Tp * s.N, int(ldg)), dtype=torch.float32, device=w.device)
    call("ds2_ctc_multi_backward", P(s.rows), P(s.offs), P(s.lens), P(s.il), s.Tp, s.N, s.R, s.Cc, s.blank, s.mtl, P(w), P(dlogits),
         int(ldg), P(s.ws), S())
    return dlogits


def mwer_weights(nll, err, K, has_ref, ce_weight):
    """The MWER rule on the device (ds2_mwer_weights).  nll [(K + has_ref)][N] f32 of ctc_multi_forward, err [K][N] int32 error
    counts of the K hypothesis ranks (None when K = 0).  Returns device tensors (weights, same shape as nll; risk [N]; nll_ref [N];
    loss [1])."""
    if not (torch.is_tensor(nll) and nll.is_cuda and nll.dtype == torch.float32 and nll.dim() == 2):
        raise ValueError("nll must be a float32 HIP device tensor [ranks][N]")
    K, has_ref = int(K), bool(has_ref)
    R, N = nll.shape
    if K < 0 or R != K + int(has_ref) or R < 1 or N < 1:
        raise ValueError("nll has %d ranks of %d clips for K = %d hypotheses%s" % (R, N, K, " and the reference" if has_ref else ""))
    ce_weight = float(ce_weight)
    if not 0.0 <= ce_weight <= 3.4e38:
        raise ValueError("ce_weight must be a finite value >= 0, got %r" % (ce_weight,))
    if K > 0:
        if not (torch.is_tensor(err) and err.is_cuda and err.numel() == K * N):
            raise ValueError("err must be a HIP device tensor of %d x %d error counts" % (K, N))
        err = err.to(torch.int32).contiguous()
    else:
        err = None
    dev = nll.device
    nll = nll.contiguous()
    weights = torch.empty_like(nll)
    out = torch.empty(2 * N + 1, dtype=torch.float32, device=dev)
    risk, nll_ref, loss = out[:N], out[N:2 * N], out[2 * N:]
    call("ds2_mwer_weights", P(nll), P(err), N, K, int(has_ref), ce_weight, P(weights), P(risk), P(nll_ref), P(loss), S())
    return weights, risk, nll_ref, loss


CTC_ALIGN_MAX_TARGET_LEN = 2047     # ds2_ctc_align: labels of one target
CTC_ALIGN_MODES = {"logits": 0, "probs": 1, "log_probs": 2}


def ctc_align(x, sizes, targets, target_lengths, blank=0, mode="probs", max_target_len=None):
    """CTC forced alignment (ds2_ctc_align): the best path of every clip's KNOWN target through the network's outputs.
    x: (N, T', C) float32 CUDA tensor, any strides with a contiguous class dimension (the transposed view DeepSpeech.forward returns
    is read in place); mode: what x holds, "logits", "probs" or "log_probs" (or 0, 1, 2).  sizes: [N] valid frames; targets: the
    flat concatenation of the clips' labels; target_lengths: [N]; each on the host or on the device.
    Returns device tensors (frame_state (N, T') int32, tok_start, tok_end int32 and tok_logp float32 flat like targets, score [N]
    float32); a clip without a path has score -inf, frame_state / tok_start / tok_end -1 and tok_logp 0 (include/ds2hip.h).
    No host synchronisation: with target_lengths on the host the longest target is known; with target_lengths on the device pass
    max_target_len, or the lattice is sized for min(len(targets), CTC_ALIGN_MAX_TARGET_LEN) labels.  A clip longer than that bound
    comes back without a path.  Host lengths are checked to add up to len(targets); lengths that live on the device cannot be
    checked without reading them back, so that they are >= 0 and add up to at most len(targets) is the CALLER's contract there:
    the kernel reads targets and writes the label outputs at the offsets the lengths give."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 3 and x.dtype == torch.float32):
        raise ValueError("ctc_align takes a float32 HIP device tensor of shape (N, T', C)")
    N, Tp, Cc = x.shape
    if N < 1 or Tp < 1 or Cc < 1:
        raise ValueError("ctc_align needs at least one clip, one frame and one class; got shape %s" % (tuple(x.shape),))
    m = CTC_ALIGN_MODES.get(mode, mode)
    if m not in (0, 1, 2):
        raise ValueError("mode must be one of %s, got %r" % (sorted(CTC_ALIGN_MODES), mode))
    if not 0 <= int(blank) < Cc:
        raise ValueError("blank index %d out of range for %d classes" % (blank, Cc))
    if x.stride(2) != 1:
        x = x.contiguous()
    dev = x.device
    sz = torch.as_tensor(sizes).reshape(-1)
    tlh = torch.as_tensor(target_lengths).reshape(-1)
    tg = torch.as_tensor(targets).reshape(-1)
    if sz.shape[0] != N or tlh.shape[0] != N:
        raise ValueError("sizes has %d and target_lengths %d entries for %d clips" % (sz.shape[0], tlh.shape[0], N))
    total = tg.shape[0]
    prefill = False
    if not tlh.is_cuda:                                    # host lengths: checked here, nothing is read back
        longest = int(tlh.max())
        if int(tlh.min()) < 0 or longest > CTC_ALIGN_MAX_TARGET_LEN:
            raise ValueError("a target has %d labels; ctc_align takes 0 to %d" % (longest, CTC_ALIGN_MAX_TARGET_LEN))
        if int(tlh.sum()) != total:
            raise ValueError("target_lengths add up to %d labels, targets has %d" % (int(tlh.sum()), total))
        if max_target_len is None:
            max_target_len = longest
        elif max_target_len < longest:
            raise ValueError("max_target_len is %d, the longest target has %d labels" % (max_target_len, longest))
    elif max_target_len is None:
        max_target_len = min(total, CTC_ALIGN_MAX_TARGET_LEN)
        prefill = total > CTC_ALIGN_MAX_TARGET_LEN         # a clip beyond the cap leaves its label entries untouched
    if not 0 <= int(max_target_len) <= CTC_ALIGN_MAX_TARGET_LEN:
        raise ValueError("max_target_len must be in [0, %d], got %d" % (CTC_ALIGN_MAX_TARGET_LEN, max_target_len))
    max_target_len = int(max_target_len)
    sz = sz.to(dev, torch.int32).contiguous()
    tl = tlh.to(dev, torch.int32).contiguous()
    tg = tg.to(dev, torch.int32).contiguous()
    if total == 0:                                         # every target is empty: the entry still takes a non-null pointer
        tg = torch.zeros(1, dtype=torch.int32, device=dev)
    offs = (torch.cumsum(tl, 0, dtype=torch.int32) - tl).contiguous()
    frame_state = torch.empty((N, Tp), dtype=torch.int32, device=dev)
    tok = torch.empty((2, max(total, 1)), dtype=torch.int32, device=dev)
    tok_logp = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
    if prefill:
        tok.fill_(-1)
        tok_logp.zero_()
    score = torch.empty(N, dtype=torch.float32, device=dev)
    ws = torch.empty(query("ds2_ctc_align_ws_bytes", Tp, N, max_target_len), dtype=torch.uint8, device=dev)
    call("ds2_ctc_align", P(x), x.stride(0), x.stride(1), N, Tp, Cc, m, P(sz), P(tg), P(offs), P(tl), max_target_len, int(blank),
         P(frame_state), P(tok[0]), P(tok[1]), P(tok_logp), P(score), P(ws), S())
    return frame_state, tok[0, :total], tok[1, :total], tok_logp[:total], score


# ---- keyword spotting (csrc/ds2_kws.hip) ----------------------------------------------------------------------------------------
KWS_MAX_LABELS, KWS_MAX_HITS, KWS_MAX_STREAMS = 64, 4096, 65535     # ds2_kws_feed's limits
KWS_FIRST_FETCH = 32          # hits per stream that travel with the headers; a feed with more costs a second copy


class KwsHandle:
    """The device state of N keyword spotters (ds2_kws_*) over one packed keyword list.  Made by kws_open."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def kws_open(num_streams, lanes, num_keywords, hold, max_hits, blank, device="cuda"):
    """Opens N = num_streams spotters.  lanes: the packing of the K = num_keywords keywords, an int32 array
    (waves * 64, 4) of (label, flags, keyword, thr_abs bits) per lane (keywords.pack).  The handle owns
    ds2_kws_state_bytes(N, waves, K) bytes of state and the output rows (N, ds2_kws_out_stride(K, max_hits)) int32.  Every
    stream starts at frame 0 with no path."""
    N, K, hold, max_hits = int(num_streams), int(num_keywords), int(hold), int(max_hits)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("a keyword spotter lives on a HIP device, not on %s" % dev)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if not 1 <= N <= KWS_MAX_STREAMS:
        raise ValueError("a keyword stream takes 1 to %d streams, got %d" % (KWS_MAX_STREAMS, N))
    if hold < 1 or not 1 <= max_hits <= KWS_MAX_HITS or K < 1 or int(blank) < 0:
        raise ValueError("kws_open needs hold >= 1, max_hits in [1, %d], keywords and a blank >= 0; got %d, %d, %d, %d"
                         % (KWS_MAX_HITS, hold, max_hits, K, blank))
    ln = torch.as_tensor(np.ascontiguousarray(lanes, dtype=np.int32))
    if ln.dim() != 2 or ln.shape[1] != 4 or ln.shape[0] == 0 or ln.shape[0] % 64:
        raise ValueError("lanes is an int32 array of shape (waves * 64, 4), got %s" % (tuple(ln.shape),))
    W = ln.shape[0] // 64
    with torch.cuda.device(dev):
        state = torch.empty(query("ds2_kws_state_bytes", N, W, K) // 4, dtype=torch.int32, device=dev)
        stride = query("ds2_kws_out_stride", K, max_hits)
        h = KwsHandle(state=state, key=state[N * W * 256:N * W * 256 + N * K * 8].view(N, K, 8),
                      frm=state[N * W * 256 + N * K * 8:N * W * 256 + N * K * 8 + N * W].view(N, W), lanes=ln.to(dev), N=N, W=W, K=K,
                      hold=hold, max_hits=max_hits, blank=int(blank), device=dev,
                      out=torch.empty((N, stride), dtype=torch.int32, device=dev))
        kws_reset(h)
    return h


def kws_reset(h, streams=None):
    """Streams `streams` (indices; None = all) start again: no path, no candidate, no best, frame 0; the others are untouched."""
    call("ds2_kws_reset", P(h.state), h.N, h.W, h.K, P(_stream_mask(streams, h.N, h.device)), S())


def kws_feed(h, x, sizes=None, mode="probs", end=None):
    """Advances the spotters of h over one chunk and fetches the hits that THIS feed emits (ds2_kws_feed; waits for the device).
    x: (N, Tc, C) float32 CUDA tensor, any strides with a contiguous class dimension (the transposed view DeepSpeech.forward
    returns is read in place), or None for an end alone; mode: what x holds, "logits", "probs" or "log_probs"; sizes: [N] ints
    (tensor or sequence; None = Tc), frames at and beyond them are never read and 0 leaves a stream as it is.  end: None, True
    (every stream ends after its frames: an open candidate is emitted) or the indices of the streams that end.
    Returns (hits, dropped): per stream the list of (keyword, start_frame, end_frame, score) in (keyword, time) order with
    absolute frames, and the hits of this feed beyond max_hits per keyword, which are counted and not returned."""
    N, K = h.N, h.K
    m = CTC_ALIGN_MODES.get(mode, mode)
    if m not in (0, 1, 2):
        raise ValueError("mode must be one of %s, got %r" % (sorted(CTC_ALIGN_MODES), mode))
    if x is None:
        Tc, Cc, xs = 0, 2 ** 31 - 1, (P(None), 0, 0)       # no column is read; every label counts as a class
    else:
        if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 3 and x.dtype == torch.float32 and x.shape[0] == N
                and x.shape[2] > h.blank):
            raise ValueError("a chunk for this keyword stream is a float32 HIP device tensor of shape (%d, Tc, C > %d), got %s"
                             % (N, h.blank, tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
        if x.stride(2) != 1:
            x = x.contiguous()
        Tc, Cc = x.shape[1], x.shape[2]
        xs = (P(x), x.stride(0), x.stride(1)) if Tc > 0 else (P(None), 0, 0)
    sz = _sizes_to_device(sizes, h.device) if Tc > 0 else None
    if sz is not None and sz.shape != (N,):
        raise ValueError("sizes must have one entry per stream (%d), got shape %s" % (N, tuple(sz.shape)))
    end_all = end is True
    mask = None if end is None or end_all else _stream_mask(end, N, h.device)
    if Tc == 0 and not end_all and mask is None:
        return [[] for _ in range(N)], [0] * N
    ws = torch.empty(query("ds2_kws_ws_bytes", N, Tc, K, h.max_hits), dtype=torch.uint8, device=h.device)
    call("ds2_kws_feed", *xs, N, Tc, Cc, m, P(sz), h.blank, P(h.lanes), h.W, K, h.hold, h.max_hits, P(mask), int(end_all),
         P(h.state), P(h.out), P(ws), S())
    first = min(K * h.max_hits, KWS_FIRST_FETCH)
    host = h.out[:, :4 + 4 * first].cpu()
    counts = host[:, 0].tolist()
    top = max(counts)
    rows = host[:, 4:]
    if top > first:
        rows = torch.cat([rows, h.out[:, 4 + 4 * first:4 + 4 * top].cpu()], 1)
    hits = []
    for n in range(N):
        r = rows[n, :4 * counts[n]].view(counts[n], 4)
        sc = r[:, 3].contiguous().view(torch.float32).tolist()
        hits.append([(k, b, e, s) for (k, b, e, _), s in zip(r.tolist(), sc)])
    return hits, host[:, 1].tolist()


def kws_best(h):
    """Host tensors (scores (N, K) float32, spans (N, K, 2) int32): per stream and keyword the largest end score so far and its
    (start, end) frames; -inf, -1, -1 before any path exists (waits for the device)."""
    key = h.key.cpu()
    return key[:, :, 3].contiguous().view(torch.float32), key[:, :, 4:6].contiguous()


def kws_frames(h):
    """Frames consumed per stream (host ints; waits for the device)."""
    return h.frm[:, 0].cpu().tolist()


# ---- word timings and confidence (csrc/ds2_confidence.hip) --------------------------------------------------------------------
CONFIDENCE_MAX_CLASSES, CONFIDENCE_MAX_BEAMS = 8192, 256     # ds2_confidence's limits (the decoders')
CONFIDENCE_MEASURES = {"label_prob": 0, "max_prob": 1, "entropy": 2, "tsallis": 3, "renyi": 4}
CONFIDENCE_AGGREGATES = {"mean": 0, "min": 1, "prod": 2}


def confidence(x, sizes, tokens, offsets, lens, blank, space, measure="label_prob", alpha=1 / 3, aggregate="mean",
               word_aggregate="min", kind="probs", t0=None, cap=None):
    """Spans, word tables and confidences of hypotheses that live on the device (ds2_confidence; the rules are in
    include/ds2hip.h).  x: (N, T', C) float32 CUDA tensor as the decoders take it, `kind` as ctc_align's mode; sizes: [N] or None.
    tokens, offsets: (N, B, ld) int32 CUDA tensors, lens (N, B): the hypotheses as a decoder's device buffers hold them.  space:
    the space label (>= C: none).  t0 / cap: frame t of row n is row (t0[n] + t) % cap of x, a stream's ring; then T' = cap
    frames at most are addressed and sizes is required.  Returns ten device tensors: tok_start, tok_end, tok_conf (N, B, ld);
    word_first, word_last, word_start, word_end, word_conf (N, B, (ld + 1) // 2); word_count, utt_conf (N, B).  No host
    synchronisation."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 3 and x.dtype == torch.float32):
        raise ValueError("confidence takes a float32 HIP device tensor of shape (N, T', C)")
    N, Tp, Cc = x.shape
    if Cc > CONFIDENCE_MAX_CLASSES:
        raise ValueError("at most %d classes, got %d" % (CONFIDENCE_MAX_CLASSES, Cc))
    if N < 1 or Tp < 1 or Cc < 1:
        raise ValueError("confidence needs at least one clip, one frame and one class; got shape %s" % (tuple(x.shape),))
    k = CTC_ALIGN_MODES.get(kind, kind)
    if k not in (0, 1, 2):
        raise ValueError("kind must be one of %s, got %r" % (sorted(CTC_ALIGN_MODES), kind))
    m = CONFIDENCE_MEASURES.get(measure, measure)
    ag, wag = CONFIDENCE_AGGREGATES.get(aggregate, aggregate), CONFIDENCE_AGGREGATES.get(word_aggregate, word_aggregate)
    if m not in range(5) or ag not in range(3) or wag not in range(3):
        raise ValueError("measure must be one of %s and the aggregates of %s, got %r, %r, %r"
                         % (sorted(CONFIDENCE_MEASURES), sorted(CONFIDENCE_AGGREGATES), measure, aggregate, word_aggregate))
    alpha = float(alpha)
    if not alpha > 0:
        raise ValueError("alpha must be > 0, got %r" % (alpha,))
    if m >= 3 and alpha == 1:
        raise ValueError("alpha == 1 is not an order of the tsallis or renyi entropy")
    if m >= 2 and Cc < 2:
        raise ValueError("at least 2 classes for an entropy measure, got %d" % Cc)
    if not 0 <= int(blank) < Cc:
        raise ValueError("blank index %d out of range for %d classes" % (blank, Cc))
    if int(space) < 0:
        raise ValueError("space label %d must be >= 0 (the number of classes or more: no space label)" % space)
    for name, t in (("tokens", tokens), ("offsets", offsets)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.dim() == 3 and t.shape[0] == N):
            raise ValueError("%s must be an int32 HIP device tensor of shape (N, B, ld)" % name)
    B, ld = tokens.shape[1], tokens.shape[2]
    if B > CONFIDENCE_MAX_BEAMS:
        raise ValueError("at most %d hypotheses per clip, got %d" % (CONFIDENCE_MAX_BEAMS, B))
    if B < 1 or ld < 1 or offsets.shape != tokens.shape or tuple(lens.shape) != (N, B):
        raise ValueError("tokens %s, offsets %s and lens %s do not describe (N, B, ld >= 1) hypotheses"
                         % (tuple(tokens.shape), tuple(offsets.shape), tuple(lens.shape)))
    if (t0 is None) != (cap is None) or (t0 is not None and sizes is None):
        raise ValueError("a ring is addressed with t0, cap and sizes together")
    if x.stride(2) != 1:
        x = x.contiguous()
    dev = x.device
    if t0 is not None:
        if int(cap) != Tp:
            raise ValueError("cap=%d must be the rows of the store, %d" % (cap, Tp))
        t0 = t0.to(dev, torch.int32).contiguous()
    sz = sizes.to(dev, torch.int32).contiguous() if sizes is not None else None
    tokens, offsets, lens = tokens.contiguous(), offsets.contiguous(), lens.to(dev, torch.int32).contiguous()
    lw = (ld + 1) // 2
    tok_i = torch.empty((2, N, B, ld), dtype=torch.int32, device=dev)
    tok_c = torch.empty((N, B, ld), dtype=torch.float32, device=dev)
    word_i = torch.empty((4, N, B, lw), dtype=torch.int32, device=dev)
    word_c = torch.empty((N, B, lw), dtype=torch.float32, device=dev)
    count = torch.empty((N, B), dtype=torch.int32, device=dev)
    utt = torch.empty((N, B), dtype=torch.float32, device=dev)
    ws = torch.empty(query("ds2_confidence_ws_bytes", N, Tp), dtype=torch.uint8, device=dev)
    call("ds2_confidence", P(x), x.stride(0), x.stride(1), N, Tp, Cc, k, P(sz), P(t0), Tp, P(tokens), P(offsets), P(lens), B, ld, lw,
         int(blank), int(space), m, alpha, ag, wag, P(tok_i[0]), P(tok_i[1]), P(tok_c), P(word_i[0]), P(word_i[1]), P(word_i[2]),
         P(word_i[3]), P(word_c), P(count), P(utt), P(ws), S())
    return tok_i[0], tok_i[1], tok_c, word_i[0], word_i[1], word_i[2], word_i[3], word_c, count, utt


def _words_to_host(x, sz, tokens, offsets, lens, blank, wc, kind="probs", t0=None, cap=None):
    """The confidence pass on a decode's own device buffers, then the one trip to the host: tokens, offsets (N, B, ld) and lens
    (N, B) on the device; wc = dict(space, measure, alpha, aggregate, word_aggregate, nbest).  Only the top nbest ranks are passed
    and come back.  Returns (labels[n][r], offsets[n][r] as lists, res[n][r] = the hypothesis' rows of confidence's ten outputs as
    host lists / numbers, cut to its length and word count)."""
    N, B = lens.shape
    R = max(1, min(int(wc["nbest"]), B))
    tk, of, ln = tokens[:, :R], offsets[:, :R], lens[:, :R]
    out = confidence(x, sz, tk, of, ln, blank, wc["space"], wc["measure"], wc["alpha"], wc["aggregate"], wc["word_aggregate"], kind,
                     t0, cap)
    lnh, cnt = ln.cpu().numpy(), out[8].cpu().numpy()
    width, wwidth = max(int(lnh.max()), 1), max(int(cnt.max()), 1)
    ih = torch.stack([tk[:, :, :width], of[:, :, :width], out[0][:, :, :width], out[1][:, :, :width]]).cpu().numpy()
    tch = out[2][:, :, :width].cpu().numpy()
    wih = torch.stack([o[:, :, :wwidth] for o in out[3:7]]).cpu().numpy()
    wch, utt = out[7][:, :, :wwidth].cpu().numpy(), out[9].cpu().numpy()
    labels, offs, res = [], [], []
    for n in range(N):
        labels.append([ih[0, n, r, :max(lnh[n, r], 0)].tolist() for r in range(R)])
        offs.append([ih[1, n, r, :max(lnh[n, r], 0)].tolist() for r in range(R)])
        res.append([(ih[2, n, r, :max(lnh[n, r], 0)].tolist(), ih[3, n, r, :max(lnh[n, r], 0)].tolist(),
                     tch[n, r, :max(lnh[n, r], 0)].tolist(), wih[0, n, r, :cnt[n, r]].tolist(), wih[1, n, r, :cnt[n, r]].tolist(),
                     wih[2, n, r, :cnt[n, r]].tolist(), wih[3, n, r, :cnt[n, r]].tolist(), wch[n, r, :cnt[n, r]].tolist(),
                     int(cnt[n, r]), float(utt[n, r])) for r in range(R)])
    return labels, offs, res


class FrameStore:
    """The frames a stream keeps for the confidence pass: rows (N, cap, C) float32 and the frames stored so far, count [N] int32,
    both on the device.  Made by frame_store_open."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def frame_store_open(num_streams, cap, num_classes, device="cuda"):
    """A store of cap frames of num_classes classes for each of num_streams streams (4 * num_classes bytes per frame and stream);
    frame f of a stream lives at row f % cap."""
    N, cap, Cc = int(num_streams), int(cap), int(num_classes)
    if N < 1 or cap < 1 or not 1 <= Cc <= CONFIDENCE_MAX_CLASSES:
        raise ValueError("a frame store needs num_streams >= 1, cap >= 1 and 1 to %d classes, got %d, %d and %d"
                         % (CONFIDENCE_MAX_CLASSES, N, cap, Cc))
    return FrameStore(rows=torch.zeros((N, cap, Cc), dtype=torch.float32, device=device),
                      count=torch.zeros(N, dtype=torch.int32, device=device), N=N, cap=cap, C=Cc)


def frame_store_append(store, x, sizes=None):
    """Appends the first sizes[n] (device int32 tensor; None = all) frames of chunk x (N, Tc, C) to every stream's rows
    (ds2_frame_store_append).  No host synchronisation.  A chunk longer than cap goes in pieces."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 3 and x.dtype == torch.float32 and x.shape[0] == store.N
            and x.shape[2] == store.C and x.stride(2) == 1):
        raise ValueError("a chunk for this store is a float32 HIP device tensor of shape (%d, Tc, %d)" % (store.N, store.C))
    for t0 in range(0, x.shape[1], store.cap):
        part = x[:, t0:t0 + store.cap]
        sz = None if sizes is None else (sizes - t0).clamp_(0, part.shape[1])
        call("ds2_frame_store_append", P(part), part.stride(0), part.stride(1), store.N, part.shape[1], store.C, P(sz), P(store.count),
             P(store.rows), store.cap, S())


def frame_store_reset(store, streams=None):
    """Streams `streams` (None = all) start again at frame 0."""
    if streams is None:
        store.count.zero_()
    else:
        store.count[torch.tensor([int(n) for n in streams], dtype=torch.long, device=store.count.device)] = 0


def beam_stream_words(h, store, row_stride, wc, sizes=None, t0=None):
    """_words_to_host on the beams of every stream of h for the frames consumed so far, read from `store`; returns its three
    values and the host scores and acoustic (N, nbest).  The state is left unchanged.  sizes, t0 (device int32 [N]): the frames
    are an endpointed stream's open segment, sizes[n] frames from row t0[n] of the ring; default: the store from its row 0."""
    N, B = h.N, h.B
    R = 1 if int(wc["nbest"]) == 1 else B
    row_stride = max(int(row_stride), 1)
    buf, lens, scores = _beam_outputs(N, R, row_stride, h.device)
    _beam_stream_launch(h, None, 0, None, buf, lens, scores, row_stride, R)
    sc = scores.cpu()
    plain = h.lm is None and h.hot is None
    if t0 is None:
        res = _words_to_host(store.rows, store.count, buf[0], buf[1], lens, h.blank, wc)
    else:
        res = _words_to_host(store.rows, sizes, buf[0], buf[1], lens, h.blank, wc, "probs", t0, store.cap)
    return res + (sc[0], sc[0] if plain else sc[1])


def ring_segments_words(store, groups, blank, wc, kind="probs"):
    """The confidence pass for segments of streams whose frames live in the ring `store`, their hypotheses on the host.  groups:
    a list of (sizes, starts, hyps): for every stream n one segment of sizes[n] frames (0: none) that began at absolute frame
    starts[n], with hyps[n] = [(labels, offsets from the segment's start)] * B; several groups when a stream has several
    segments.  Everything is uploaded in ONE copy (a pinned int32 buffer), then one ds2_confidence call per group.  Returns
    _words_to_host's value per group."""
    N, G = store.N, len(groups)
    B = len(groups[0][2][0])
    ld = max(1, max(len(t) for _, _, hyps in groups for hs in hyps for t, _ in hs))
    per = 2 * N + N * B * (2 * ld + 1)
    pack = torch.zeros(G * per, dtype=torch.int32).pin_memory()
    for g, (sizes, starts, hyps) in enumerate(groups):
        p = pack[g * per:(g + 1) * per]
        p[:N] = torch.as_tensor(sizes, dtype=torch.int32)
        p[N:2 * N] = torch.as_tensor([int(s) % store.cap for s in starts], dtype=torch.int32)
        tk, of = p[2 * N:2 * N + N * B * ld].view(N, B, ld), p[2 * N + N * B * ld:2 * N + 2 * N * B * ld].view(N, B, ld)
        ln = p[2 * N + 2 * N * B * ld:].view(N, B)
        for n, hs in enumerate(hyps):
            for b, (t, o) in enumerate(hs):
                tk[n, b, :len(t)] = torch.as_tensor(t, dtype=torch.int32)
                of[n, b, :len(t)] = torch.as_tensor(o, dtype=torch.int32)
                ln[n, b] = len(t)
    dev = pack.to(store.rows.device, non_blocking=True)
    out = []
    for g in range(G):
        p = dev[g * per:(g + 1) * per]
        tk, of = p[2 * N:2 * N + N * B * ld].view(N, B, ld), p[2 * N + N * B * ld:2 * N + 2 * N * B * ld].view(N, B, ld)
        out.append(_words_to_host(store.rows, p[:N], tk, of, p[2 * N + 2 * N * B * ld:].view(N, B), blank, dict(wc, nbest=B), kind,
                                  p[N:2 * N], store.cap))
    return out


def host_hypotheses_words(x, sizes, hyps, blank, wc, kind="probs", t0=None, cap=None):
    """_words_to_host for hypotheses that live on the host: hyps[n] = [(labels, offsets)] * B as lists.  They are uploaded in ONE
    copy (tokens, offsets and lengths packed in one pinned int32 buffer)."""
    N, B = len(hyps), len(hyps[0])
    ld = max(1, max(len(t) for hs in hyps for t, _ in hs))
    pack = torch.zeros(N * B * (2 * ld + 1), dtype=torch.int32).pin_memory()
    tk, of, ln = pack[:N * B * ld].view(N, B, ld), pack[N * B * ld:2 * N * B * ld].view(N, B, ld), pack[2 * N * B * ld:].view(N, B)
    for n, hs in enumerate(hyps):
        for b, (t, o) in enumerate(hs):
            tk[n, b, :len(t)] = torch.as_tensor(t, dtype=torch.int32)
            of[n, b, :len(t)] = torch.as_tensor(o, dtype=torch.int32)
            ln[n, b] = len(t)
    dev = pack.to(x.device, non_blocking=True)
    tk, of, ln = dev[:N * B * ld].view(N, B, ld), dev[N * B * ld:2 * N * B * ld].view(N, B, ld), dev[2 * N * B * ld:].view(N, B)
    return _words_to_host(x, sizes, tk, of, ln, blank, dict(wc, nbest=B), kind, t0, cap)


# ---- waveform augmentation (csrc/ds2_waveaug.hip) ---------------------------------------------------------------------------
def _wave_batch(wav, nsamples):
    if not (torch.is_tensor(wav) and wav.is_cuda and wav.dim() == 2 and wav.dtype == torch.float32):
        raise ValueError("the waveform kernels take a float32 HIP device batch of shape (N, Lmax)")
    ns = torch.as_tensor(nsamples).to(wav.device, torch.int32).reshape(-1).contiguous()
    if ns.shape[0] != wav.shape[0]:
        raise ValueError("nsamples has %d entries for %d clips" % (ns.shape[0], wav.shape[0]))
    return wav.contiguous(), ns


def _per_clip(a, N, dev, dtype, what):
    if a is None:
        return None
    a = torch.as_tensor(a).to(dev, dtype).reshape(-1).contiguous()
    if a.shape[0] != N:
        raise ValueError("%s has %d entries for %d clips" % (what, a.shape[0], N))
    return a


def wsola(wav, nsamples, tempo, ldo, Smax, out=None):
    """Tempo change at constant pitch of every clip of wav (N, Lmax) (clip n = its first nsamples[n] samples) by the per-clip
    factors tempo [N] (None = copy): ds2_wsola.  ldo / Smax: row length of the output and of the offsets (the largest
    augment.wsola_out_len / wsola_segments of the batch).  Returns (out (N, ldo), nsamples_out [N] int32, offsets (N, Smax) int32),
    all on the device; entries of out beyond a clip's own samples are zero."""
    wav, ns = _wave_batch(wav, nsamples)
    N = wav.shape[0]
    tp = _per_clip(tempo, N, wav.device, torch.float32, "tempo")
    if out is None:
        out = torch.empty((N, int(ldo)), dtype=torch.float32, device=wav.device)
    if tuple(out.shape) != (N, int(ldo)) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("out must be a contiguous float32 (N, ldo) tensor")
    ns_out = torch.empty(N, dtype=torch.int32, device=wav.device)
    offsets = torch.empty((N, int(Smax)), dtype=torch.int32, device=wav.device)
    call("ds2_wsola", P(wav), wav.stride(0), P(ns), P(tp), N, P(out), int(ldo), P(ns_out), P(offsets) if Smax else P(None), int(Smax), S())
    return out, ns_out, offsets


def resample(wav, nsamples, taps, up, down, half_width, ldo, out=None):
    """Every clip of wav (N, Lmax) (clip n = its first nsamples[n] samples) through the polyphase filter taps (up, 2 half_width) f32
    on the device, `up` outputs per `down` inputs: ds2_resample.  ldo: row length of the output (the largest out_len of the batch).
    Returns (out (N, ldo), nsamples_out [N] int32), both on the device; entries of out beyond a clip's own outputs are zero."""
    wav, ns = _wave_batch(wav, nsamples)
    N = wav.shape[0]
    if out is None:
        out = torch.empty((N, int(ldo)), dtype=torch.float32, device=wav.device)
    if tuple(out.shape) != (N, int(ldo)) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("out must be a contiguous float32 (N, ldo) tensor")
    ns_out = torch.empty(N, dtype=torch.int32, device=wav.device)
    call("ds2_resample", P(wav), wav.stride(0), P(ns), N, P(taps), int(up), int(down), int(half_width), P(out), int(ldo), P(ns_out), S())
    return out, ns_out


def resample_stream_feed(wav, rows, n_rows, max_new, max_emit, capacity, taps, up, down, half_width, state):
    """One feed of n_rows streams through the polyphase filter: ds2_resample_stream_feed.  wav (.., L) f32 chunks (None for
    max_new = 0), rows = the device table of ds2_resample_stream_row, state = the carries of `capacity` slots.  Returns out
    (n_rows, max_emit) f32: row r holds its emit outputs, zero beyond them."""
    dev = state.device
    out = torch.empty((n_rows, int(max_emit)), dtype=torch.float32, device=dev)
    ws = torch.empty(query("ds2_resample_stream_ws_bytes", n_rows, int(half_width)), dtype=torch.uint8, device=dev)
    call("ds2_resample_stream_feed", P(wav) if max_new else P(None), wav.stride(0) if max_new else 0, P(rows), n_rows, int(max_new),
         int(max_emit), int(capacity), P(taps), int(up), int(down), int(half_width), P(state), P(out) if max_emit else P(None),
         int(max_emit), P(ws), S())
    return out


def resample_mixed(wav, nsamples, cls, classes, classes_dev, taps, ldo, out=None):
    """Every clip of wav (N, Lmax) through the polyphase filter of ITS class, one launch: ds2_resample_mixed.  nsamples / cls: [N]
    int32 on the device (sample counts, class per row); classes: the host's class table (int32 numpy, 10 words a class, as
    ds2_resample_classes filled it), classes_dev / taps: the same table and the concatenated tap tables on the device.  Returns
    (out (N, ldo), nsamples_out [N] int32), both on the device; entries of out beyond a clip's own outputs are zero."""
    if not (torch.is_tensor(wav) and wav.is_cuda and wav.dim() == 2 and wav.dtype == torch.float32):
        raise ValueError("the waveform kernels take a float32 HIP device batch of shape (N, Lmax)")
    wav, N = wav.contiguous(), wav.shape[0]
    for t, what in ((nsamples, "nsamples"), (cls, "cls")):
        if not (t.is_cuda and t.dtype == torch.int32 and t.numel() == N and t.is_contiguous()):
            raise ValueError("%s must be a contiguous int32 device tensor with one entry per clip" % what)
    if out is None:
        out = torch.empty((N, int(ldo)), dtype=torch.float32, device=wav.device)
    if tuple(out.shape) != (N, int(ldo)) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("out must be a contiguous float32 (N, ldo) tensor")
    ns_out = torch.empty(N, dtype=torch.int32, device=wav.device)
    call("ds2_resample_mixed", P(wav), wav.stride(0), P(nsamples), P(cls), N, C.c_void_p(classes.ctypes.data), P(classes_dev),
         classes.size // 10, P(taps), P(out), int(ldo), P(ns_out), S())
    return out, ns_out


def resample_stream_feed_mixed(wav, rows, n_rows, max_new, max_emit, capacity, classes, classes_dev, taps, wmax, state):
    """One feed of n_rows streams, each through the filter of its row's class: ds2_resample_stream_feed_mixed.  As
    resample_stream_feed; the class travels in the row table, state = the carries [capacity][2 wmax]."""
    dev = state.device
    out = torch.empty((n_rows, int(max_emit)), dtype=torch.float32, device=dev)
    ws = torch.empty(query("ds2_resample_stream_ws_bytes_mixed", n_rows, int(wmax)), dtype=torch.uint8, device=dev)
    call("ds2_resample_stream_feed_mixed", P(wav) if max_new else P(None), wav.stride(0) if max_new else 0, P(rows), n_rows, int(max_new),
         int(max_emit), int(capacity), C.c_void_p(classes.ctypes.data), P(classes_dev), classes.size // 10, P(taps), int(wmax), P(state),
         P(out) if max_emit else P(None), int(max_emit), P(ws), S())
    return out


def _noise_args(N, dev, level, bank, noise_off, noise_start):
    lv = _per_clip(level, N, dev, torch.float32, "level")
    if lv is None:
        return None, None, 0, None, None
    if bank is None or noise_off is None or noise_start is None:
        raise ValueError("noise levels need a noise bank with per-clip offsets and starts")
    if not (bank.is_cuda and bank.dtype == torch.float32 and bank.dim() == 1 and bank.is_contiguous()):
        raise ValueError("the noise bank is a contiguous 1-D float32 HIP device tensor")
    return (lv, bank, bank.numel(), _per_clip(noise_off, N, dev, torch.int64, "noise_off"),
            _per_clip(noise_start, N, dev, torch.int32, "noise_start"))


def wave_energy(wav, nsamples, gain=None, level=None, bank=None, noise_off=None, noise_start=None):
    """Per clip the sum of squares of clamp(gain * x) and of its noise crop as fixed-order fp64 partials (N, 8, 2): ds2_wave_energy.
    Their sum over axis 1 is (data energy, noise energy); the noise column is zero for a clip without noise."""
    wav, ns = _wave_batch(wav, nsamples)
    N = wav.shape[0]
    g = _per_clip(gain, N, wav.device, torch.float32, "gain")
    lv, bank, blen, off, start = _noise_args(N, wav.device, level, bank, noise_off, noise_start)
    nbytes = query("ds2_wave_ws_bytes", N)
    partial = torch.empty((N, nbytes // (16 * N), 2), dtype=torch.float64, device=wav.device)
    call("ds2_wave_energy", P(wav), wav.stride(0), P(ns), N, P(g), P(lv), P(bank), blen, P(off), P(start), P(partial), S())
    return partial


def wave_mix(wav, nsamples, gain=None, level=None, bank=None, noise_off=None, noise_start=None, partial=None, out=None):
    """out = clamp(gain * x, -1, 1) + level * rms(data) / rms(noise) * noise crop for every clip of wav (N, Lmax): ds2_wave_energy
    (unless its `partial` is handed in, or no clip gets noise) + ds2_wave_mix.  gain [N] LINEAR factors (None = samples unchanged
    and not clamped), level [N] (None = no noise), bank = the 1-D device noise buffer, noise_off [N] int64 (negative = no noise for
    the clip), noise_start [N].  Returns a new (N, Lmax) tensor (or fills `out`, (N, ldo)), zero beyond a clip's own samples."""
    wav, ns = _wave_batch(wav, nsamples)
    N = wav.shape[0]
    g = _per_clip(gain, N, wav.device, torch.float32, "gain")
    lv, bank, blen, off, start = _noise_args(N, wav.device, level, bank, noise_off, noise_start)
    if lv is not None and partial is None:
        partial = wave_energy(wav, ns, g, lv, bank, off, start)
    if out is None:
        out = torch.empty_like(wav)
    if out.dim() != 2 or out.shape[0] != N or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("out must be a contiguous float32 (N, ldo) tensor")
    call("ds2_wave_mix", P(wav), wav.stride(0), P(ns), N, P(g), P(lv), P(bank), blen, P(off), P(start),
         P(partial if lv is not None else None), P(out), out.shape[1], S())
    return out


def reverb(wav, nsamples, bank, rir_off, rir_len, rir_peak, out=None):
    """Every clip of wav (N, Lmax) convolved with its room impulse response, aligned on the response's peak tap and cut to the
    clip's length: out[i] = sum_k h[k] x[i + peak - k], ds2_reverb (csrc/ds2_reverb.hip).  bank = the 1-D device buffer of the
    responses (augment.RirBank.samples), rir_off [N] int64 (negative = the clip is copied; None = every clip is copied and bank /
    rir_len / rir_peak may be None), rir_len / rir_peak [N] int32.  Returns a new (N, Lmax) tensor (or fills `out`, (N, ldo)), zero
    beyond a clip's own samples."""
    wav, ns = _wave_batch(wav, nsamples)
    N = wav.shape[0]
    off = _per_clip(rir_off, N, wav.device, torch.int64, "rir_off")
    ln = pk = None
    if off is not None:
        if bank is None or rir_len is None or rir_peak is None:
            raise ValueError("rir_off needs the bank of responses with per-clip lengths and peaks")
        if not (bank.is_cuda and bank.dtype == torch.float32 and bank.dim() == 1 and bank.is_contiguous()):
            raise ValueError("the bank of responses is a contiguous 1-D float32 HIP device tensor")
        ln = _per_clip(rir_len, N, wav.device, torch.int32, "rir_len")
        pk = _per_clip(rir_peak, N, wav.device, torch.int32, "rir_peak")
    else:
        bank = None
    if out is None:
        out = torch.empty_like(wav)
    if out.dim() != 2 or out.shape[0] != N or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("out must be a contiguous float32 (N, ldo) tensor")
    # the row length, not stride(0): a contiguous one-row view may carry any stride there
    call("ds2_reverb", P(wav), wav.shape[1], P(ns), N, P(bank), bank.numel() if bank is not None else 0, P(off), P(ln), P(pk),
         P(out), out.shape[1], S())
    return out


# ---- exact chunked inference (csrc/ds2_stream.hip, streaming.StreamingTranscriber(carry_context=True)) ----------------------
STREAM_CONV_CARRY = 10     # positions both convolutions carry: their kernel width in time minus one


def stream_state_views(dtype, N, F0, H, ctx, device):
    """The double-buffered carries of one session in ONE zeroed buffer of ds2_stream_state_bytes: ([2][N][F0][10] f32 input frames,
    [2][N][F1][10][32] conv1 activations, [2][ctx-1][N][H] RNN rows (None for ctx = 1)) as lists of the two views, and the buffer."""
    nbytes = query("ds2_stream_state_bytes", dt(dtype), N, F0, H, ctx)
    if nbytes <= 0:
        raise ValueError("ds2_stream_state_bytes refuses dtype %s, N %d, F0 %d, H %d, ctx %d" % (dtype, N, F0, H, ctx))
    buf = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    F1 = conv_rows(F0)[0]
    views, pos = [], 0
    for shape, d in (((N, F0, STREAM_CONV_CARRY), torch.float32), ((N, F1, STREAM_CONV_CARRY, 32), dtype), ((ctx - 1, N, H), dtype)):
        n = int(np.prod(shape)) * (4 if d == torch.float32 else 2)
        pair = []
        for _ in range(2):
            pair.append(buf[pos:pos + n].view(d).view(shape) if n else None)
            pos += rup(n, 256)
        views.append(pair)
    assert pos == nbytes, (pos, nbytes)
    return views[0], views[1], views[2], buf


def stream_conv1(x, carry, nxt, w1k, b1, scale, shift, off, J, dtype, lens=None, live=None):
    """conv1 + eval BatchNorm + Hardtanh over the window [carry | x]: x (N, 1, F0, Tc) f32 (Tc may be 0), carry / nxt [N][F0][10] f32.
    Returns the J new activation frames [N][F1][J][32] in `dtype`; nxt receives the next carry."""
    N, _, F0, Tc = x.shape
    y = torch.empty((N, conv_rows(F0)[0], J, 32), dtype=dtype, device=x.device)
    call("ds2_stream_conv1", dt(dtype), PF(x) if Tc else C.c_void_p(0), PF(carry), PF(nxt), PF(w1k), PF(b1), PF(scale), PF(shift),
         P(lens), P(live), P(y) if J else C.c_void_p(0), N, F0, Tc, off, J, S())
    return y


def stream_conv2(a1, carry, nxt, w2t, b2, scale, shift, off, J, rld, F0=161, lens=None, live=None, out=None):
    """conv2 + eval BatchNorm + Hardtanh over the window [carry | a1]: a1 [N][F1][Jin][32], carry / nxt [N][F1][10][32].  Returns the
    J new rows of the sequence layout, X0 [(j*N + n)][rld] (written into `out` when given); nxt receives the next carry."""
    N, F1, Jin, _ = a1.shape
    assert F1 == conv_rows(F0)[0] and carry.dtype == a1.dtype == nxt.dtype == w2t.dtype
    x0 = torch.empty((J * N, rld), dtype=a1.dtype, device=a1.device) if out is None else out
    assert tuple(x0.shape) == (J * N, rld) and x0.is_contiguous() and x0.dtype == a1.dtype
    call("ds2_stream_conv2", dt(a1), P(a1) if Jin else C.c_void_p(0), P(carry), P(nxt), P(w2t), PF(b2), PF(scale), PF(shift),
         P(lens), P(live), P(x0) if J else C.c_void_p(0), N, F0, Jin, off, J, rld, S())
    return x0


def stream_lookahead(x, carry, nxt, w, N, H, off, J, lens=None):
    """hardtanh(lookahead) over the window of rows [carry ctx-1 | x Jin][N][H]; w [H][ctx] f32.  Returns the J new output rows
    [J*N][H]; nxt receives the next carry (carry / nxt None for ctx = 1)."""
    ctx, Jin = w.shape[1], x.shape[0] // N
    y = torch.empty((J * N, H), dtype=x.dtype, device=x.device)
    call("ds2_stream_lookahead", dt(x), P(x) if Jin else C.c_void_p(0), P(carry), P(nxt), PF(w), P(lens), P(y) if J else C.c_void_p(0),
         N, H, ctx, Jin, off, J, S())
    return y


# ---- ... for a pool of streams that start and end on their own (streaming.StreamPool) --------------
STREAM_ROW_WORDS = 16      # int32 words of one ds2_stream_row: slot, src, cur, fresh, len, off1, cnt1, off2, cnt2, off3, cnt3, 5 reserved
_STREAM_STAGING = PinnedRing()


def stream_rows(rows, S, n_src, Tc, device):
    """The row table of one feed on the device, through pinned memory in one queued copy.  rows: per batch row the 11 ints of a
    ds2_stream_row (slot, src, cur, fresh, len, off1, cnt1, off2, cnt2, off3, cnt3), already in launch order (cnt2 descending).
    Checks on the host what the kernels cannot refuse: distinct slots in [0, S), src in [0, n_src), len in [0, Tc], counts and
    offsets >= 0, cnt3 > 0 only with cnt2 > 0.  Returns (table [n][16] int32, cnt2 [n] int32, slots [n] int64) device tensors,
    views of one buffer."""
    t = np.zeros((len(rows), STREAM_ROW_WORDS), dtype=np.int32)
    if len(rows) == 0:
        raise ValueError("a feed needs at least one row")
    t[:, :11] = np.asarray(rows, dtype=np.int64).reshape(len(rows), 11)
    slot, src, cur, fresh = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    if slot.min() < 0 or slot.max() >= S or len(set(slot.tolist())) != len(rows):
        raise ValueError("row slots must be distinct and lie in [0, %d), got %s" % (S, slot.tolist()))
    if src.min() < 0 or src.max() >= n_src:
        raise ValueError("source rows must lie in [0, %d), got %s" % (n_src, src.tolist()))
    if ((cur | fresh) & ~7).any() or t[:, 4].min() < 0 or t[:, 4].max() > Tc or t[:, 5:11].min() < 0:
        raise ValueError("bad row table (bits beyond the three stages, a length outside [0, %d] or a negative offset or count):\n%s"
                         % (Tc, t[:, :11]))
    cnt2 = t[:, 8]
    if (np.diff(cnt2) > 0).any() or ((t[:, 10] > 0) & (cnt2 == 0)).any():
        raise ValueError("rows must be ordered by cnt2 descending, and only a row with RNN frames has output frames: cnt2 %s, cnt3 %s"
                         % (cnt2.tolist(), t[:, 10].tolist()))
    n = len(rows)
    pad = np.zeros((n * (STREAM_ROW_WORDS + 1)) % 2, dtype=np.int32)                 # the int64 slots start on 8 bytes
    buf = _STREAM_STAGING.stage(device, [t.reshape(-1), cnt2, pad, slot.astype(np.int64).view(np.int32)])
    o = n * STREAM_ROW_WORDS
    return buf[:o].view(n, STREAM_ROW_WORDS), buf[o:o + n], buf[o + n + pad.size:].view(torch.int64)


def stream_conv1_rows(x, carry, rows, w1k, b1, scale, shift, J, dtype):
    """stream_conv1 by the row table: x (n_src, 1, F0, Tc) f32 as the caller holds it (row r reads x[src]), carry the pool's two
    buffers [S][F0][10] f32, rows the device table [n][16].  Returns [n][F1][J][32] in `dtype`, in table order."""
    _, _, F0, Tc = x.shape
    n = rows.shape[0]
    y = torch.empty((n, conv_rows(F0)[0], J, 32), dtype=dtype, device=x.device)
    call("ds2_stream_conv1_rows", dt(dtype), PF(x) if Tc else C.c_void_p(0), PF(carry[0]), PF(carry[1]), P(rows), PF(w1k), PF(b1),
         PF(scale), PF(shift), P(y) if J else C.c_void_p(0), n, F0, Tc, J, S())
    return y


def stream_conv2_rows(a1, carry, rows, n_rnn, w2t, b2, scale, shift, J, rld, F0=161, out=None):
    """stream_conv2 by the row table: a1 [n][F1][Jin][32] (stream_conv1_rows' result), carry the pool's two buffers
    [S][F1][10][32].  Returns the sequence layout of the first n_rnn rows, X0 [(j*n_rnn + r)][rld]."""
    n, F1, Jin, _ = a1.shape
    assert F1 == conv_rows(F0)[0] and carry[0].dtype == a1.dtype == carry[1].dtype == w2t.dtype and rows.shape[0] == n
    x0 = torch.empty((J * n_rnn, rld), dtype=a1.dtype, device=a1.device) if out is None else out
    assert tuple(x0.shape) == (J * n_rnn, rld) and x0.is_contiguous() and x0.dtype == a1.dtype
    call("ds2_stream_conv2_rows", dt(a1), P(a1) if Jin else C.c_void_p(0), P(carry[0]), P(carry[1]), P(rows), P(w2t), PF(b2), PF(scale),
         PF(shift), P(x0) if J else C.c_void_p(0), n, n_rnn, F0, Jin, J, rld, S())
    return x0


def stream_lookahead_rows(x, carry, rows, w, n_rnn, S_, H, J):
    """stream_lookahead by the row table over its first n_rnn rows: x [Jin*n_rnn][H], carry the pool's two buffers [ctx-1][S_][H]
    (None, None for ctx = 1).  Returns [J*n_rnn][H]."""
    ctx, Jin = w.shape[1], x.shape[0] // n_rnn
    y = torch.empty((J * n_rnn, H), dtype=x.dtype, device=x.device)
    call("ds2_stream_lookahead_rows", dt(x), P(x) if Jin else C.c_void_p(0), P(carry[0]), P(carry[1]), P(rows), PF(w),
         P(y) if J else C.c_void_p(0), n_rnn, S_, H, ctx, Jin, J, S())
    return y
