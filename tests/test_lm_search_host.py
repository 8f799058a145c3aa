"""Host checks of the language-model weight search: the grid workspace query, the chunk planner, LMGridSearch's points, results,
best and save from injected counters, and the argument errors that need no device."""
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm")
SHAPES = [(1, 2, 1), (3, 17, 10), (32, 751, 128)]


def _lib():
    from deepspeech.pytorch_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("N,T,B", SHAPES)
def test_grid_workspace_of_one_point_is_the_plain_workspace(N, T, B):
    lib = _lib()
    assert lib.ds2_beam_grid_ws_bytes(1, N, T, B) == lib.ds2_beam_ws_bytes(N, T, B) > 0


@pytest.mark.parametrize("N,T,B", SHAPES)
def test_grid_workspace_is_affine_in_the_points(N, T, B):
    lib = _lib()
    one = lib.ds2_beam_grid_ws_bytes(1, N, T, B)
    step = lib.ds2_beam_grid_ws_bytes(2, N, T, B) - one
    assert step >= 3 * 4 * N * (T + 1) * B                # three int32 arrays of N * (T + 1) * B nodes
    assert step < one                                      # the kept lists are not repeated
    for G in (3, 7, 64, 500):
        assert lib.ds2_beam_grid_ws_bytes(G, N, T, B) == one + (G - 1) * step
    for bad in ((0, N, T, B), (-1, N, T, B), (2, 0, T, B), (2, N, 0, B), (2, N, T, 0), (2, N, -5, B)):
        assert lib.ds2_beam_grid_ws_bytes(*bad) == 0


@pytest.mark.parametrize("G,one,per,cap", [(1, 100, 40, 100), (9, 100, 40, 100), (9, 100, 40, 139), (9, 100, 40, 180), (9, 100, 40, 10 ** 9),
                                           (500, 7_000_000, 3_000_000, 1 << 30), (10, 5, 0, 5)])
def test_chunk_planner_covers_every_point_once_in_order_within_the_cap(G, one, per, cap):
    from deepspeech.pytorch_amd.ops import plan_grid_chunks
    chunks = plan_grid_chunks(G, one, per, cap)
    covered = [g for start, count in chunks for g in range(start, start + count)]
    assert covered == list(range(G))
    assert all(count >= 1 and one + (count - 1) * per <= cap for _, count in chunks)
    widest = 1 + (cap - one) // per if per else G
    assert len(chunks) == -(-G // min(widest, G))          # no more chunks than the cap asks for


def test_chunk_planner_errors_and_launch_limit():
    from deepspeech.pytorch_amd.ops import plan_grid_chunks
    with pytest.raises(ValueError, match="max_ws_bytes"):
        plan_grid_chunks(4, 101, 40, 100)
    with pytest.raises(ValueError, match="at least one point"):
        plan_grid_chunks(0, 10, 4, 100)
    assert plan_grid_chunks(10, 10, 1, 10 ** 9, max_points=4) == [(0, 4), (4, 4), (8, 2)]


def test_from_ranges_is_alpha_major():
    from deepspeech.pytorch_amd.lm_search import LMGridSearch
    s = LMGridSearch.from_ranges(0.0, 2.0, 3, 0.0, 1.0, 2)
    assert s.points == [(0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0), (2.0, 0.0), (2.0, 1.0)]
    assert LMGridSearch.from_ranges(0.5, 3.0, 1, 0.25, 1.0, 1).points == [(0.5, 0.25)]
    with pytest.raises(ValueError, match="n_alpha"):
        LMGridSearch.from_ranges(0.0, 1.0, 0, 0.0, 1.0, 2)


def _injected():
    from deepspeech.pytorch_amd.lm_search import LMGridSearch
    s = LMGridSearch(None, [(0.0, 0.0), (1.0, 0.5), (2.0, 0.5), (1.5, 2.0)])
    s.char_err = torch.tensor([30, 7, 9, 7])
    s.word_err = torch.tensor([12, 3, 3, 5])
    s.ref_chars = torch.tensor([41])
    s.ref_words = torch.tensor([9])
    return s


def test_results_best_and_ties_from_injected_counters():
    s = _injected()
    rows = s.results()
    assert rows == [[0.0, 0.0, float(12) / 9 * 100, float(30) / 41 * 100], [1.0, 0.5, float(3) / 9 * 100, float(7) / 41 * 100],
                    [2.0, 0.5, float(3) / 9 * 100, float(9) / 41 * 100], [1.5, 2.0, float(5) / 9 * 100, float(7) / 41 * 100]]
    assert s.best() == rows[1] and s.best("wer") == rows[1]       # points 1 and 2 tie on WER, points 1 and 3 on CER
    assert s.best("cer") == rows[1]
    s.word_err = torch.tensor([3, 12, 3, 3])
    assert s.best() == s.results()[0]
    with pytest.raises(ValueError, match="metric"):
        s.best("ser")


def test_rates_without_any_reference_use_a_total_of_one():
    from deepspeech.pytorch_amd.lm_search import LMGridSearch
    s = LMGridSearch(None, [(1.0, 1.0), (2.0, 2.0)])
    assert s.results() == [[1.0, 1.0, 0.0, 0.0], [2.0, 2.0, 0.0, 0.0]]
    s.char_err, s.word_err = torch.tensor([2, 0]), torch.tensor([1, 0])
    s.ref_chars, s.ref_words = torch.tensor([0]), torch.tensor([0])
    assert s.results()[0][2:] == [100.0, 200.0] and s.best() == [2.0, 2.0, 0.0, 0.0]


def test_save_writes_the_list_that_select_lm_params_loads(tmp_path):
    s = _injected()
    path = str(tmp_path / "search.json")
    s.save(path)
    with open(path) as f:
        loaded = json.load(f)
    assert isinstance(loaded, list) and all(isinstance(r, list) and len(r) == 4 for r in loaded)
    assert loaded == s.results()
    assert min(loaded, key=lambda x: x[2]) == s.best()             # select_lm_params.py's choice


def test_value_errors_that_need_no_device():
    from deepspeech.pytorch_amd.configs import LABELS
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    from deepspeech.pytorch_amd.lm_search import LMGridSearch
    with pytest.raises(ValueError, match="at least one"):
        LMGridSearch(None, [])
    plain = BeamCTCDecoder(LABELS)
    with pytest.raises(ValueError, match="lm_path"):
        LMGridSearch(plain, [(1.0, 1.0)])
    with pytest.raises(ValueError, match="lm_path"):
        plain.decode_grid(torch.zeros(1, 2, len(LABELS)), None, [(1.0, 1.0)])
    with pytest.raises(ValueError, match="at least one"):
        BeamCTCDecoder(LABELS, os.path.join(GOLDEN, "toy3.arpa")).decode_grid(torch.zeros(1, 2, len(LABELS)), None, [])
    with pytest.raises(ValueError, match="decoder"):
        LMGridSearch(None, [(1.0, 1.0)]).update(None, None, None, None)
