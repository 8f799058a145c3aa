"""The conv kernels of csrc/ds2_conv.hip bit for bit on integer operands (tests/conv_exact_cases.py has the method, the operands, the
float64 reference and the tile arithmetic; tests/test_conv_exact_host.py pins them without a device).

Every product and partial sum is an integer below 2^24, so the fp32 sums are exact in any order: an fp32 output equals the reference
in every element, a bf16 output equals its round-to-nearest-even bf16.  Compared as storage words; no tolerance, no exempted element.
Two things the tolerance tests of test_gpu_kernels.py cannot do: see a single wrong product among the 7 392 of a conv2 output in bf16
storage, and hold the second and third tile of a persistent workgroup (k_conv_rtap, k_conv1_fwd_mfma, k_conv1_wgrad_mfma) and the
chunk loop of k_conv1_wgrad to a reference.  Every case asserts the tile regime it is there for, from the device's CU count."""
import pytest
import torch

import conv_exact_cases as X
from fixtures import DEV

pytestmark = pytest.mark.gpu

DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16}


def ops():
    from deepspeech.pytorch_amd import ops as _ops
    return _ops


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def poison(*blocks):
    """NaN-filled blocks of the sizes the wrappers are about to torch.empty(), released again: the caching allocator hands the same
    memory back, so an element a kernel fails to write (an idle split of a partial-sum workspace, a masked frame) shows."""
    for numel, dtype in blocks:
        torch.full((int(numel),), float("nan"), dtype=dtype, device=DEV)
    torch.cuda.synchronize()


def check(name, got, want, dtype):
    bad = X.mismatch(got, X.expected(want, dtype))
    assert bad is None, "%s: %s" % (name, bad)


def conv1_device_operands(case, dtype):
    x = case["x"].to(torch.float32).to(DEV)
    w1k = X.conv1_weight_layout(case["w"]).to(torch.float32).to(DEV)
    return dict(x=x, w1k=w1k, b=case["b"].to(torch.float32).to(DEV), lens=torch.from_numpy(case["lens"]).to(DEV),
                dy=X.nftc(case["dy"]).to(dtype).to(DEV))


def conv1_run(case, d, dtype):
    o = ops()
    F1 = X.conv_rows(case["F0"])[0]
    poison((case["N"] * F1 * case["Tp"] * 32, dtype))
    y = o.conv1_fwd(d["x"], d["w1k"], d["b"], d["lens"], case["Tp"], dtype)
    poison((o.query("ds2_conv1_wgrad_ws_floats", case["N"], case["F0"], case["Tp"]), torch.float32))
    dw = o.conv1_wgrad(d["x"], d["dy"], case["Tp"])
    return y, dw


def conv1_exact(F0, N, T, dtype):
    assert X.conv_rows(F0) == ops().conv_rows(F0)
    case = X.conv1_operands(F0, N, T)
    ref = X.reference(case, need_dx=False)
    y, dw = conv1_run(case, conv1_device_operands(case, dtype), dtype)
    assert tuple(y.shape) == (N, X.conv_rows(F0)[0], case["Tp"], 32) and y.dtype == dtype
    check("conv1 forward", y, X.nftc(ref["y"]), dtype)
    check("conv1 weight gradient", dw, X.conv1_weight_layout(ref["dw"]), torch.float32)


def conv2_device_operands(case, dtype):
    w2d = [w.to(dtype).to(DEV) for w in X.conv2_dgrad_weight_layouts(case["w"])]
    return dict(a1=X.nftc(case["x"]).to(dtype).to(DEV), w2t=X.conv2_weight_layout(case["w"]).to(dtype).to(DEV),
                b=case["b"].to(torch.float32).to(DEV), lens=torch.from_numpy(case["lens"]).to(DEV),
                dy=X.nftc(case["dy"]).to(dtype).to(DEV), w2d=w2d)


def conv2_run(case, d, dtype):
    o = ops()
    F0, (F1, F2) = case["F0"], X.conv_rows(case["F0"])
    poison((case["N"] * F2 * case["Tp"] * 32, dtype))
    y = o.conv2_fwd(d["a1"], d["w2t"], d["b"], d["lens"], F0)
    poison((case["N"] * F1 * case["Tp"] * 32, dtype))
    dx = o.conv2_dgrad(d["dy"], d["w2d"][0], d["w2d"][1], F0)
    poison((o.query("ds2_conv2_wgrad_ws_floats", case["N"], case["Tp"]), torch.float32))
    dw = o.conv2_wgrad(d["dy"], d["a1"], F0)
    return y, dx, dw


def conv2_exact(F0, N, Tp, dtype):
    """forward, data gradient and weight gradient of one shape from one reference computation"""
    assert X.conv_rows(F0) == ops().conv_rows(F0)
    case = X.conv2_operands(F0, N, Tp)
    ref = X.reference(case, need_dx=True)
    y, dx, dw = conv2_run(case, conv2_device_operands(case, dtype), dtype)
    F1, F2 = X.conv_rows(F0)
    assert tuple(y.shape) == (N, F2, Tp, 32) and tuple(dx.shape) == (N, F1, Tp, 32) and y.dtype == dtype and dx.dtype == dtype
    check("conv2 forward", y, X.nftc(ref["y"]), dtype)
    check("conv2 data gradient", dx, X.nftc(ref["dx"]), dtype)
    check("conv2 weight gradient", dw, X.conv2_weight_layout(ref["dw"]).reshape(231, 32, 32), torch.float32)


def conv2_batch(n256, Tp, want):
    """the batch that reaches regime `want` on this device, asserted for all three k_conv_rtap launch shapes"""
    cus = cu_count()
    N = X.batch_for(X.rtap_regimes, want, Tp, cus, n256)
    assert N is not None, "no batch size puts k_conv_rtap into regime %r at T' = %d on %d CUs" % (want, Tp, cus)
    tiles = [X.rtap_tiles(N, Tp, U) for U in (41, 40)]
    print("k_conv_rtap N=%d T'=%d: %d (U = 41) / %d (U = 40) tiles on %d CUs: %s; k_conv2_wgrad_bf16d: %d items, %d tiles per row, %d splits"
          % (N, Tp, tiles[0], tiles[1], cus, want, X.wgrad_bf16d_items(N, Tp), X.cdiv(Tp, X.CWD_TB), X.CWR_SPLITS))
    assert X.rtap_regimes(N, Tp, cus) == {want}, (tiles, cus)
    return N


def conv1_batch(n256, T, want):
    cus, Tp = cu_count(), X.out_frames(T)
    N = X.batch_for(X.conv1_mfma_regimes, want, Tp, cus, n256)
    assert N is not None, "no batch size puts the conv1 MFMA kernels into regime %r at T = %d on %d CUs" % (want, T, cus)
    tiles = X.conv1_mfma_tiles(N, Tp)
    print("k_conv1_fwd_mfma / k_conv1_wgrad_mfma N=%d T=%d T'=%d: %d tiles on %d CUs: %s" % (N, T, Tp, tiles, cus, want))
    assert X.conv1_mfma_regimes(N, Tp, cus) == {want}, (tiles, cus)
    # (the weight gradient's grid is min(tiles, CUs) as well: its other cap, the blocks of k_conv1_wgrad's workspace, is no lower)
    assert min(X.conv1_wgrad_chunks(N, 81, Tp), X.C1W_MAXBLOCKS) >= min(tiles, cus)
    return N


# ---- bf16 at 161 bins: the matrix-pipe kernels ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n256,Tp,want", X.CONV2_BF16)
def test_conv2_bf16_rtap_and_row_group_wgrad_are_exact(n256, Tp, want):
    """k_conv_rtap<11>, <10> (forward: two launches through the fp32 partial sums; dgrad: even and odd rows) and k_conv2_wgrad_bf16d.
    The last row block of the forward (rows 40..43 of 41) is in every case."""
    N = conv2_batch(n256, Tp, want)
    if (n256, Tp) == (1, 1):
        assert X.wgrad_bf16d_items(N, Tp) < X.CWR_SPLITS                  # idle splits have to write zeros
    if want == "three":
        assert X.cdiv(Tp, X.CWD_TB) == 3 and X.wgrad_bf16d_items(N, Tp) > X.CWR_SPLITS
    conv2_exact(161, N, Tp, torch.bfloat16)


@pytest.mark.parametrize("n256,T,want", X.CONV1_BF16)
def test_conv1_bf16_mfma_fwd_and_wgrad_are_exact(n256, T, want):
    """k_conv1_fwd_mfma and k_conv1_wgrad_mfma: one, two and three 9-row x 128-frame tiles per workgroup"""
    N = conv1_batch(n256, T, want)
    conv1_exact(161, N, T, torch.bfloat16)


# ---- fp32 and the general kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", X.CONV1_F32_T)
def test_conv1_fp32_is_exact_at_the_64_frame_tile(T):
    """k_conv1_fwd<float>, k_conv1_wgrad<float>: T' = 64 and 65"""
    assert X.conv1_wgrad_chunks(2, 81, X.out_frames(T)) <= X.C1W_MAXBLOCKS
    conv1_exact(161, 2, T, torch.float32)


@pytest.mark.parametrize("Tp", X.CONV2_F32_TP)
def test_conv2_fp32_is_exact_at_the_tile_seams(Tp):
    """k_conv_tap<float, 1> forward (32 positions), k_conv_tap<float, 2> dgrad (64), k_conv2_wgrad<float> (CW_TB = 128)"""
    conv2_exact(161, 2, Tp, torch.float32)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("F0", X.OTHER_F0)
def test_conv1_other_geometries_are_exact_in_both_storage_types(F0, dtype):
    """k_conv1_fwd<T>, k_conv1_wgrad<T> in fp32 and bf16 storage.  F0 = 9: 5 output rows, a full row block and one of a single row."""
    assert X.conv1_wgrad_chunks(X.OTHER_N, X.conv_rows(F0)[0], X.OTHER_TP) <= X.C1W_MAXBLOCKS
    conv1_exact(F0, X.OTHER_N, X.OTHER_T, DTYPES[dtype])


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("F0", X.OTHER_F0)
def test_conv2_other_geometries_are_exact_in_both_storage_types(F0, dtype):
    """k_conv_tap<T, 1> forward, k_conv_tap<T, 2> dgrad, k_conv2_wgrad<T> in fp32 and bf16 storage.  F0 = 9: 5 and 3 rows, fewer than
    a 4-row tile and than the kernel height; the data gradient covers 3 even and 2 odd rows."""
    conv2_exact(F0, X.OTHER_N, X.OTHER_TP, DTYPES[dtype])


@pytest.mark.parametrize("dtype,F0,N,T,chunks", X.CONV1_CHUNK_LOOP)
def test_conv1_wgrad_chunk_loop_past_its_block_cap_is_exact(dtype, F0, N, T, chunks):
    """k_conv1_wgrad<T> launches at most 1 024 blocks: here some of them take a second chunk"""
    got = X.conv1_wgrad_chunks(N, X.conv_rows(F0)[0], X.out_frames(T))
    print("k_conv1_wgrad<%s> F0=%d N=%d T=%d: %d chunks on %d blocks" % (dtype, F0, N, T, got, X.C1W_MAXBLOCKS))
    assert got == chunks and X.regime(got, X.C1W_MAXBLOCKS) == "two"
    conv1_exact(F0, N, T, DTYPES[dtype])


# ---- determinism ---------------------------------------------------------------------------------------------------------------
def test_largest_bf16_cases_repeat_bit_identically():
    n256, Tp, want = X.CONV2_BF16[-1]
    case = X.conv2_operands(161, conv2_batch(n256, Tp, want), Tp)
    d = conv2_device_operands(case, torch.bfloat16)
    first, second = conv2_run(case, d, torch.bfloat16), conv2_run(case, d, torch.bfloat16)
    for name, a, b in zip(("conv2 forward", "conv2 data gradient", "conv2 weight gradient"), first, second):
        assert X.mismatch(b, a) is None, "%s, second call against the first: %s" % (name, X.mismatch(b, a))
    n256, T, want = X.CONV1_BF16[-1]
    case = X.conv1_operands(161, conv1_batch(n256, T, want), T)
    d = conv1_device_operands(case, torch.bfloat16)
    first, second = conv1_run(case, d, torch.bfloat16), conv1_run(case, d, torch.bfloat16)
    for name, a, b in zip(("conv1 forward", "conv1 weight gradient"), first, second):
        assert X.mismatch(b, a) is None, "%s, second call against the first: %s" % (name, X.mismatch(b, a))
