"""The epilogue of csrc/ds2_gemm8.hip (g8_tile) on exact operands: A and B in {-1, 0, 1}, an integer bias in [-64, 64], K in {64, 128}.
Every output is an integer of magnitude <= 192 -- exact in fp32 and in bf16 -- so the host's integer product is the expected result
bit for bit, whatever the store path: the bf16 tile through LDS (row segments of 16 bytes and the scalar column tail where
N % 8 == 4), the direct path (a leading dimension that is no multiple of 8; fp32 as float4 or as scalars), tile rows past M, a second
tile row and column, a row list, and the mixed launch (weight gradients + dX).  C is a column window of a wider buffer pre-filled with
a sentinel: what the launch must not write -- columns >= N, unlisted rows, rows >= M of the last tile -- still holds it afterwards."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -1000.0          # exact in bf16, outside [-192, 192]


def _ints(shape, lo, hi, seed):
    return np.random.RandomState(seed).randint(lo, hi + 1, shape).astype(np.int64)


def _dev_bf16(a):
    return torch.from_numpy(a.astype(np.float32)).to(DEV).to(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def _expect(values, dtype):
    """Integer array -> the tensor the device must hold, in its output type (every value is exact there)."""
    return torch.from_numpy(values.astype(np.float32)).to(dtype)


def _ldcs(N):
    """Leading dimensions of C: one that is a multiple of 8 (bf16: the path through LDS), one that is a multiple of 4 and not of 8
    (direct path; fp32 leaves as float4), an odd one (direct path, scalar stores)."""
    lds_path = (N + 7) // 8 * 8 + 8
    direct = N + 4 if (N + 4) % 8 else N + 8
    assert lds_path % 8 == 0 and direct % 8 == 4
    return lds_path, direct, N + 5


@pytest.mark.parametrize("N", [8, 260, 264, 520])
@pytest.mark.parametrize("M", [1, 255, 257, 513])
def test_nt_entry_every_store_path(M, N):
    from deepspeech.pytorch_amd import ops
    for K in (64, 128):
        a, b, bias = _ints((M, K), -1, 1, 11 + M), _ints((N, K), -1, 1, 13 + N), _ints((N,), -64, 64, 17 + N)
        A, B, bv = _dev_bf16(a), _dev_bf16(b), torch.from_numpy(bias.astype(np.float32)).to(DEV)
        prod = a @ b.T
        for dtype in (torch.bfloat16, torch.float32):
            for with_bias in (False, True):
                want = _expect(prod + bias[None, :] if with_bias else prod, dtype)
                for ldc in _ldcs(N):
                    buf = torch.full((M + 3, ldc), SENTINEL, dtype=dtype, device=DEV)
                    got = ops.gemm8_nt(A, B, bias=bv if with_bias else None, out=buf[:M, :N])
                    where = (M, N, K, dtype, with_bias, ldc)
                    assert got.data_ptr() == buf.data_ptr() and got.stride(0) == ldc
                    assert torch.equal(_bits(buf[:M, :N]), _bits(want)), where
                    assert bool((buf[:M, N:] == SENTINEL).all()) and bool((buf[M:] == SENTINEL).all()), where


@pytest.mark.parametrize("M", [1, 255, 257, 513])
def test_nt_entry_row_list(M):
    """n_phys = M + 37 physical rows, an ascending subset of M of them listed: listed rows exact, every other row untouched."""
    from deepspeech.pytorch_amd import ops
    n_phys, N = M + 37, 264
    rows_h = np.sort(np.random.RandomState(23 + M).permutation(n_phys)[:M]).astype(np.int32)
    rows = torch.from_numpy(rows_h).to(DEV)
    listed = np.zeros(n_phys, dtype=bool)
    listed[rows_h] = True
    for K in (64, 128):
        a, b, bias = _ints((n_phys, K), -1, 1, 29 + M), _ints((N, K), -1, 1, 31), _ints((N,), -64, 64, 37)
        A, B, bv = _dev_bf16(a), _dev_bf16(b), torch.from_numpy(bias.astype(np.float32)).to(DEV)
        prod = a @ b.T + bias[None, :]
        for dtype in (torch.bfloat16, torch.float32):
            want = _expect(prod[listed], dtype)
            for ldc in _ldcs(N):
                buf = torch.full((n_phys, ldc), SENTINEL, dtype=dtype, device=DEV)
                ops.gemm8_nt(A, B, bias=bv, rows=rows, out=buf[:, :N])
                where = (M, K, dtype, ldc)
                lm = torch.from_numpy(listed).to(DEV)
                assert torch.equal(_bits(buf[lm][:, :N]), _bits(want)), where
                assert bool((buf[~lm] == SENTINEL).all()) and bool((buf[:, N:] == SENTINEL).all()), where


@pytest.mark.parametrize("K_nt", [64, 128])
def test_mixed_entry_weight_gradients_and_dx(K_nt):
    """Two TN problems (256 x 264 and 512 x 8, fp32) over a ragged contraction of 130 listed rows, and the dX product (bf16) over the
    same row list, in one launch."""
    from deepspeech.pytorch_amd import ops
    n_rows, n_phys, N_nt = 130, 167, 264
    rows_h = np.sort(np.random.RandomState(41).permutation(n_phys)[:n_rows]).astype(np.int32)
    rows = torch.from_numpy(rows_h).to(DEV)
    shapes = [(256, 264), (512, 8)]
    ats = [_ints((n_phys, m), -1, 1, 43 + i) for i, (m, n) in enumerate(shapes)]
    bts = [_ints((n_phys, n), -1, 1, 47 + i) for i, (m, n) in enumerate(shapes)]
    probs = [dict(At=_dev_bf16(at), Bt=_dev_bf16(bt), M=m, N=n, lda=m, ldb=n) for at, bt, (m, n) in zip(ats, bts, shapes)]
    ax, bx = _ints((n_phys, K_nt), -1, 1, 53), _ints((N_nt, K_nt), -1, 1, 59)
    outs, dx = ops.gemm8_tn_grouped(probs, n_phys, dx=(_dev_bf16(ax), _dev_bf16(bx)), rows=rows)
    for at, bt, o in zip(ats, bts, outs):
        assert o.dtype == torch.float32
        assert torch.equal(_bits(o), _bits(_expect(at[rows_h].T @ bt[rows_h], torch.float32))), tuple(o.shape)
    assert dx.dtype == torch.bfloat16 and tuple(dx.shape) == (n_phys, N_nt)
    assert torch.equal(_bits(dx[rows.long()]), _bits(_expect((ax @ bx.T)[rows_h], torch.bfloat16)))
    # the grouped entry without dX: the same weight gradients
    for o, o2 in zip(outs, ops.gemm8_tn_grouped(probs, n_phys, rows=rows)):
        assert torch.equal(_bits(o), _bits(o2))
