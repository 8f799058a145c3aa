"""Host half of the exact conv tests (tests/conv_exact_cases.py; the device half is tests/test_gpu_conv_exact.py): the float64 torch
reference is pinned to the project's oracle, every case of the tables has integer references below 2^24 (what makes the device
comparison exact), and the tile arithmetic puts every case, on 256 compute units, in the regime its comment claims."""
import numpy as np
import pytest
import torch

import conv_exact_cases as X
from oracle import ds2_oracle as O


def _np(t):
    return t.detach().numpy()


@pytest.mark.parametrize("layer,F0,N,T", [("conv1", 161, 1, 1), ("conv1", 9, 2, 80), ("conv2", 161, 1, 1), ("conv2", 9, 2, 40)])
def test_torch_reference_equals_the_oracle(layer, F0, N, T):
    """Integer operands: the oracle's float64 matrix products are exact too, so the two agree in every element, not within a bound."""
    case = X.conv1_operands(F0, N, T) if layer == "conv1" else X.conv2_operands(F0, N, T)
    ref = X.reference(case, need_dx=True)
    stride, pad = case["layer"]["stride"], case["layer"]["padding"]
    y = O.conv2d_fwd(_np(case["x"]), _np(case["w"]), _np(case["b"]), stride, pad)
    y[O.time_mask(y.shape, case["lens"])] = 0
    dx, dw, _ = O.conv2d_bwd(_np(case["x"]), _np(case["w"]), _np(case["dy"]), stride, pad)
    assert np.array_equal(_np(ref["y"]), y) and np.abs(y).max() > 0
    assert np.array_equal(_np(ref["dw"]), dw) and np.abs(dw).max() > 0
    assert np.array_equal(_np(ref["dx"]), dx) and np.abs(dx).max() > 0


def _check_operands(case, lo, hi):
    N, Tp, lens = case["N"], case["Tp"], case["lens"].tolist()
    assert lens == X.out_lens(N, Tp) and lens[0] == Tp and min(lens) >= 1
    seam = 32 * ((Tp - 1) // 32)
    if seam and N >= 2:
        assert seam in lens
    if seam and (N >= 3 or Tp == seam + 1):
        assert seam + 1 in lens
    if N >= 4 or Tp == 1:
        assert 1 in lens
    for name, (a, b) in (("x", (lo, hi)), ("w", (lo, hi)), ("b", (-4, 4)), ("dy", (-1, 1))):
        v = case[name]
        assert bool((v == v.round()).all()) and float(v.min()) >= a and float(v.max()) <= b, name
    live = X.time_mask(lens, Tp)[:, None, None, :]
    assert bool((case["dy"] * (1 - live) == 0).all())
    for n, L in enumerate(lens):                      # something to mask against: the last live frame of every clip is not all zero
        assert float(case["dy"][n, :, :, L - 1].abs().sum()) > 0


@pytest.mark.parametrize("F0,N,T", X.all_conv1_cases())
def test_conv1_references_are_integers_below_2_24(F0, N, T):
    case = X.conv1_operands(F0, N, T)
    _check_operands(case, -2, 2)
    for n, L in enumerate(case["lens_in"]):
        assert float(case["x"][n, :, :, L:].abs().sum()) == 0
    ref = X.reference(case, need_dx=False)               # asserts both properties
    assert tuple(ref["y"].shape) == (N, 32, X.conv_rows(F0)[0], X.out_frames(T)) and tuple(ref["dw"].shape) == (32, 1, 41, 11)
    assert X.expected(ref["dw"], torch.float32).dtype == torch.float32


@pytest.mark.parametrize("F0,N,Tp", X.all_conv2_cases())
def test_conv2_references_are_integers_below_2_24(F0, N, Tp):
    case = X.conv2_operands(F0, N, Tp)
    _check_operands(case, -1, 1)
    assert bool((case["x"] * (1 - X.time_mask(case["lens"], Tp)[:, None, None, :]) == 0).all())
    ref = X.reference(case, need_dx=True)
    F1, F2 = X.conv_rows(F0)
    assert tuple(ref["y"].shape) == (N, 32, F2, Tp) and tuple(ref["dx"].shape) == (N, 32, F1, Tp) and tuple(ref["dw"].shape) == (32, 32, 21, 11)
    if Tp > 1:                                           # the data gradient reaches beyond the shortest clip's end
        n, L = N - 1, int(case["lens"][-1])
        assert L == Tp or float(ref["dx"][n, :, :, L:].abs().sum()) > 0


def test_expected_bits_round_once_to_nearest_even():
    v = torch.tensor([0.0, -3.0, 255.0, 256.0, 257.0, 258.0, 259.0, -261.0, 309.0, 16777215.0], dtype=torch.float64)
    assert X.expected(v, torch.float32).tolist() == v.tolist()
    # bf16 keeps 8 significant bits: above 256 the grid is 2 wide, 257 and 259 and 261 are ties and go to the even neighbour
    assert X.expected(v[:9], torch.bfloat16).to(torch.float64).tolist() == [0.0, -3.0, 255.0, 256.0, 256.0, 258.0, 260.0, -260.0, 308.0]
    assert X.words(X.expected(X.assert_exact("zero", torch.tensor([-0.0], dtype=torch.float64)), torch.bfloat16)).tolist() == [0]
    with pytest.raises(AssertionError):
        X.assert_exact("half", torch.tensor([0.5], dtype=torch.float64))
    with pytest.raises(AssertionError):
        X.assert_exact("big", torch.tensor([float(1 << 24)], dtype=torch.float64))


def test_mismatch_reports_count_first_index_and_values():
    a = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4).to(torch.bfloat16)
    assert X.mismatch(a, a.clone()) is None
    b = a.clone()
    b[1, 0, 2], b[1, 2, 3] = 99.0, -1.0
    assert X.mismatch(b, a) == "2 of 24 elements differ; first at (1, 0, 2): got 99.0, want 14.0"
    z = torch.zeros(3)
    assert X.mismatch(-z, z) is not None                  # storage words: a negative zero is not a zero


def test_tile_counts_put_every_case_in_its_regime_on_256_cus():
    cus = X.CUS_OF_THE_TABLES
    for N, Tp, want in X.CONV2_BF16:
        assert X.rtap_regimes(N, Tp, cus) == {want}, (N, Tp)
        assert X.batch_for(X.rtap_regimes, want, Tp, cus, N) == N
    assert [X.rtap_tiles(3, 257, U) for U in (41, 40)] == [297, 270]
    assert [X.rtap_tiles(6, 289, U) for U in (41, 40)] == [660, 600]
    assert 257 % 32 == 1 and 289 % 32 == 1              # the last frame tile of the two multi-tile cases holds one frame
    # the largest case of tests/test_gpu_kernels.py stays single-tile
    assert X.rtap_tiles(2, 300, 41) == 220 and X.regime(220, cus) == "one"
    for N, T, want in X.CONV1_BF16:
        assert X.conv1_mfma_regimes(N, X.out_frames(T), cus) == {want}, (N, T)
        assert X.batch_for(X.conv1_mfma_regimes, want, X.out_frames(T), cus, N) == N
    assert [X.out_frames(T) for _, T, _ in X.CONV1_BF16] == [1, 128, 128, 129, 513, 769]
    assert X.conv1_mfma_tiles(8, 513) == 360 and X.conv1_mfma_tiles(12, 769) == 756 and 513 % 128 == 1 and 769 % 128 == 1
    assert X.conv1_mfma_tiles(3, X.out_frames(523)) == 81   # test_conv1_fwd_and_wgrad's largest: N = 2 at T = 523 is 54 tiles
    # the weight gradient of conv2: idle splits at the smallest shape; one tile, then a second one of a single position; three tiles
    assert X.wgrad_bf16d_items(1, 1) == 44 < X.CWR_SPLITS
    assert X.cdiv(112, X.CWD_TB) == 1 and X.cdiv(113, X.CWD_TB) == 2 and 113 - X.CWD_TB == 1
    assert X.cdiv(289, X.CWD_TB) == 3 and X.wgrad_bf16d_items(6, 289) == 792 > 9 * X.CWR_SPLITS
    # k_conv1_wgrad<T>: every other case fits its 1 024 blocks, the two chunk-loop cases do not
    for _, F0, N, T, chunks in X.CONV1_CHUNK_LOOP:
        got = X.conv1_wgrad_chunks(N, X.conv_rows(F0)[0], X.out_frames(T))
        assert got == chunks and X.regime(got, X.C1W_MAXBLOCKS) == "two"
    general = [(161, 2, T) for T in X.CONV1_F32_T] + [(F0, X.OTHER_N, X.OTHER_T) for F0 in X.OTHER_F0]
    assert all(X.conv1_wgrad_chunks(N, X.conv_rows(F0)[0], X.out_frames(T)) <= X.C1W_MAXBLOCKS for F0, N, T in general)
    assert [X.out_frames(T) for T in X.CONV1_F32_T] == [64, 65] and X.out_frames(X.OTHER_T) == X.OTHER_TP
    assert X.conv_rows(161) == (81, 41) and X.conv_rows(9) == (5, 3) and X.conv_rows(81) == (41, 21)


@pytest.mark.parametrize("cus", [120, 228, 240, 304])
def test_batch_for_reaches_the_regime_on_other_cu_counts(cus):
    for N, Tp, want in X.CONV2_BF16:
        n = X.batch_for(X.rtap_regimes, want, Tp, cus, N)
        assert n is not None and X.rtap_regimes(n, Tp, cus) == {want}, (N, Tp, want, n)
    for N, T, want in X.CONV1_BF16:
        n = X.batch_for(X.conv1_mfma_regimes, want, X.out_frames(T), cus, N)
        assert n is not None and X.conv1_mfma_regimes(n, X.out_frames(T), cus) == {want}, (N, T, want, n)


def test_regime_boundaries():
    assert [X.regime(t, 256) for t in (1, 256, 257, 511, 512, 513, 768, 769)] == ["one", "one", "two", "two", "other", "three", "three", "other"]
