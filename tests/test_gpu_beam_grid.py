"""GPU checks of the grid form of the language-model beam search (ds2_beam_decode_lm_grid, ops.beam_decode_lm_grid): row (g, n)
must be rank 0 of ops.beam_decode_lm at point g, bit for bit -- both run the same kernel code on the same input, so no tolerance
appears.  One case is also held against the numpy restatement (tests/beam_lm_reference.py), so that the grid is not pinned to
other device code alone.  Inputs and ARPA fixtures are those of tests/test_gpu_beam_lm.py."""
import functools

import numpy as np
import pytest
import torch

from beam_lm_reference import Scorer, beam_search_lm
from test_gpu_beam_lm import DEV, _inputs, _labels, _lm, _tables

pytestmark = pytest.mark.gpu

# alpha and beta in [0, 2]; (0, 0) first, one point twice
POINTS = [(0.0, 0.0), (1.3, 0.7), (1.3, 0.7), (2.0, 2.0), (0.5, 2.0), (2.0, 0.0), (0.8, 1.5), (1.0, 1.0), (0.0, 1.2)]
# (N, T, B, model, lexicon, cutoff_prob, strided (T, N, C) view, G)
CASES = [
    (1, 2, 1, "toy3", False, 1.0, False, 1),
    (3, 17, 10, "toy3", True, 1.0, True, 5),
    (3, 200, 128, "toy5", True, 0.9, False, 4),      # the lexicon and the cut leave frames without a candidate: no beam survives
    (8, 17, 256, "toy3", False, 0.9, False, 3),
    (8, 200, 10, "toy5", False, 1.0, False, 9),
]
IDS = ["-".join(str(v) for v in c) for c in CASES]


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _run(case):
    """the case's input, the grid call's five tensors and, per point, ops.beam_decode_lm's result: made once, never changed"""
    from deepspeech.pytorch_amd import ops
    N, T, B, name, lexicon, cutoff_prob, strided, G = case
    p, sizes = _inputs(N * 1000 + T * 7 + B, N, T, name)
    assert sizes[0] == T and (N < 3 or sizes[1] == 0)
    if strided:
        view = torch.from_numpy(np.ascontiguousarray(p.transpose(1, 0, 2))).to(DEV).transpose(0, 1)
        assert not view.is_contiguous()
    else:
        view = torch.from_numpy(p).to(DEV)
    wt, gt = _tables(name)
    m = _lm(name)
    sp = _labels().index(' ')
    pts = POINTS[:G]
    args = (view, torch.from_numpy(sizes), 0, B, 40, cutoff_prob, sp, wt, gt, m.order, m.bos)
    grid = ops.beam_decode_lm_grid(*args, [a for a, _ in pts], [b for _, b in pts], lexicon)
    single = [ops.beam_decode_lm(*args, a, b, lexicon) for a, b in pts]
    return p, sizes, args, pts, grid, single


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_point_equals_rank_zero_of_the_single_point_entry(case):
    N, T, B, name, lexicon, cutoff_prob, strided, G = case
    _, _, _, pts, (tokens, offsets, lens, scores, acoustic), single = _run(case)
    assert tokens.shape == (G, N, T) and offsets.shape == (G, N, T) and lens.shape == (G, N)
    assert scores.shape == (G, N) and acoustic.shape == (G, N) and tokens.is_cuda and scores.is_cuda
    tk, of, ln = tokens.cpu().numpy(), offsets.cpu().numpy(), lens.cpu().numpy()
    for g in range(G):
        toks, offs, sc, ac = single[g]
        for n in range(N):
            assert ln[g, n] == len(toks[n][0]), (g, n)
            assert tk[g, n, :ln[g, n]].tolist() == toks[n][0], (g, n)
            assert of[g, n, :ln[g, n]].tolist() == offs[n][0].tolist(), (g, n)
        assert torch.equal(_bits(scores[g]), _bits(sc[:, 0])), g            # +inf (no beam alive) included
        assert torch.equal(_bits(acoustic[g]), _bits(ac[:, 0])), g


def test_the_case_without_a_surviving_beam_has_one():
    """case 3 is there for the rank-0 row of an utterance whose beams all died"""
    single = _run(CASES[2])[5]
    scores = _run(CASES[2])[4][3].cpu()
    assert any(bool(torch.isinf(sc[:, 0]).any()) for _, _, sc, _ in single) and bool(torch.isinf(scores).any())


@pytest.mark.parametrize("case", [c for c in CASES if c[7] >= 3], ids=[i for c, i in zip(CASES, IDS) if c[7] >= 3])
def test_duplicated_points_give_identical_rows(case):
    pts, grid = _run(case)[3], _run(case)[4]
    assert pts[1] == pts[2]
    for t in grid:
        assert torch.equal(_bits(t[1]), _bits(t[2]))


@pytest.mark.parametrize("case", [c for c in CASES if not c[4]], ids=[i for c, i in zip(CASES, IDS) if not c[4]])
def test_zero_weights_in_open_mode_equal_the_entry_without_lm(case):
    from deepspeech.pytorch_amd import ops
    N, T, B, name, lexicon, cutoff_prob, strided, G = case
    _, _, args, pts, (tokens, offsets, lens, scores, acoustic), _ = _run(case)
    assert pts[0] == (0.0, 0.0)
    toks, offs, sc = ops.beam_decode(args[0], args[1], 0, B, 40, cutoff_prob)
    tk, of, ln = tokens.cpu().numpy(), offsets.cpu().numpy(), lens.cpu().numpy()
    for n in range(N):
        assert tk[0, n, :ln[0, n]].tolist() == toks[n][0] and of[0, n, :ln[0, n]].tolist() == offs[n][0].tolist(), n
    assert torch.equal(_bits(scores[0]), _bits(sc[:, 0])) and torch.equal(_bits(acoustic[0]), _bits(sc[:, 0]))


@pytest.mark.parametrize("case", [c for c in CASES if c[7] >= 3], ids=[i for c, i in zip(CASES, IDS) if c[7] >= 3])
def test_chunked_call_equals_the_unchunked_call(case):
    from deepspeech.pytorch_amd import _lib, ops
    N, T, B, name, lexicon, cutoff_prob, strided, G = case
    _, _, args, pts, grid, _ = _run(case)
    lib = _lib.load()
    one = lib.ds2_beam_grid_ws_bytes(1, N, T, B)
    cap = one + (lib.ds2_beam_grid_ws_bytes(2, N, T, B) - one) * (G // 3 - 1)        # G // 3 points a chunk: three chunks or more
    assert len(ops.plan_grid_chunks(G, one, lib.ds2_beam_grid_ws_bytes(2, N, T, B) - one, cap)) >= 3
    chunked = ops.beam_decode_lm_grid(*args, [a for a, _ in pts], [b for _, b in pts], lexicon, max_ws_bytes=cap)
    for a, b in zip(grid, chunked):
        assert torch.equal(_bits(a), _bits(b))
    with pytest.raises(ValueError, match="max_ws_bytes"):
        ops.beam_decode_lm_grid(*args, [1.0], [1.0], lexicon, max_ws_bytes=one - 1)


def test_grid_equals_the_numpy_restatement():
    case = CASES[1]
    N, T, B, name, lexicon, cutoff_prob, strided, G = case
    p, sizes, _, pts, (tokens, offsets, lens, _, _), _ = _run(case)
    tk, of, ln = tokens.cpu().numpy(), offsets.cpu().numpy(), lens.cpu().numpy()
    words = 0
    for g, (alpha, beta) in enumerate(pts):
        sc = Scorer(_lm(name), _labels(), 0, alpha, beta, lexicon, np.float32)
        for n in range(N):
            ref = beam_search_lm(p[n], sizes[n], 0, B, 40, cutoff_prob, sc)
            labels, frames = ref["beams"][0][0], ref["beams"][0][1]
            assert tuple(tk[g, n, :ln[g, n]].tolist()) == tuple(labels), (g, n)
            assert tuple(of[g, n, :ln[g, n]].tolist()) == tuple(frames), (g, n)
            words += ref["word_events"]
    assert words >= 1


def test_argument_errors_and_empty_input():
    import ctypes
    from deepspeech.pytorch_amd import _lib, ops
    N, T, B, name, lexicon, cutoff_prob, strided, G = CASES[1]
    _, _, args, pts, _, _ = _run(CASES[1])
    for bad, match in ((dict(alphas=[]), "alphas"), (dict(alphas=[1.0, 2.0], betas=[1.0]), "betas"), (dict(alphas=[[1.0]]), "alphas"),
                       (dict(beam_width=257), "beam_width"), (dict(space=0), "space"), (dict(order=6), "order")):
        kw = dict(zip(("probs", "sizes", "blank", "beam_width", "cutoff_top_n", "cutoff_prob", "space", "word_table", "ngram_table",
                       "order", "bos"), args), alphas=[1.0], betas=[1.0])
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            ops.beam_decode_lm_grid(**kw)
    empty = ops.beam_decode_lm_grid(args[0][:, :0], None, *args[2:], [0.0, 1.0], [0.0, 1.0])
    assert empty[0].shape == (2, N, 0) and empty[2].shape == (2, N) and not empty[2].any() and not empty[3].any()
    # the raw ABI
    lib = _lib.load()
    p = args[0].contiguous()
    C = p.shape[2]
    wt, gt, m = args[7], args[8], _lm(name)
    al = torch.tensor([1.0, 0.5], device=DEV)
    buf = torch.empty((2, 2, N, T), dtype=torch.int32, device=DEV)
    lens = torch.empty((2, N), dtype=torch.int32, device=DEV)
    scores = torch.empty((2, N), dtype=torch.float32, device=DEV)
    ws = torch.empty(lib.ds2_beam_grid_ws_bytes(2, N, T, B), dtype=torch.uint8, device=DEV)

    def raw(G=2, alphas=al.data_ptr(), betas=al.data_ptr(), order=m.order, space=args[6], offsets=buf[1].data_ptr()):
        return lib.ds2_beam_decode_lm_grid(p.data_ptr(), p.stride(0), p.stride(1), N, T, C, None, 0, B, 40, 1.0, space, wt.data_ptr(),
                                           wt.shape[0], gt.data_ptr(), gt.shape[0], order, m.bos, 1, G, alphas, betas,
                                           buf[0].data_ptr(), offsets, lens.data_ptr(), scores.data_ptr(), None, ws.data_ptr(),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    assert raw() == 0 and raw(offsets=None) == 0
    torch.cuda.synchronize()
    for kw in (dict(G=0), dict(G=-3), dict(alphas=None), dict(betas=None), dict(order=6), dict(space=0)):
        assert raw(**kw) == 1002, kw                                          # DS2_ERR_ARG
