"""Host-side check of how ops.py marshals the character-LM beam search's C calls, in the manner of
tests/test_beam_marshal_host.py: the launch-level functions are run on CPU tensors with ops.call recorded, and the recorded
arguments must be the ones include/ds2hip.h declares for ds2_beam_decode_clm, ds2_beam_stream_feed_clm and
ds2_beam_decode_clm_grid, in its order.  The slot count, order, bos, alpha and beta all differ, so a swapped pair shows.  Also:
every ds2_beam_*clm* declaration has one ctypes type per argument, and the stream size queries know the flag word 5 alone
beyond 0 .. 3.  No GPU needed."""
import os
import re

import pytest
import torch

from test_beam_marshal_host import (ALPHA, B, BETA, BLANK, BOS, C, CUTOFF, MAX_FRAMES, N, NGRAM_SLOTS, ORDER, ROW_STRIDE, T, TOP_N,
                                    AnyPointer, Case, check, lib, ptr, rec)

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ds2hip.h")


class CharCase(Case):
    def __init__(self):
        super().__init__()
        self.ids = torch.arange(C, dtype=torch.int32)
        self.lm = dict(unit="char", label_ids=self.ids, ngram_table=self.gt, order=ORDER, bos=BOS, alpha=ALPHA, beta=BETA)


def test_one_shot_entry_gets_the_headers_arguments(rec):
    from deepspeech.pytorch_amd import ops
    t = CharCase()
    buf, lens, scores = ops._beam_outputs(N, B, T, "cpu")
    ops._beam_launch(t.probs, t.sz, BLANK, B, TOP_N, CUTOFF, t.lm, None, buf, lens, scores, t.ws)
    # const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank, int B, int cutoff_top_n,
    # float cutoff_prob, const int* cid, const void* ngram_table, long ngram_slots, int order, int bos, float alpha, float beta,
    # int* tokens, int* offsets, int* lens, float* scores, float* acoustic, void* ws, ds2_stream_t stream
    check(rec, "ds2_beam_decode_clm", (ptr(t.probs), (T + 1) * C, C, N, T, C, ptr(t.sz), BLANK, B, TOP_N, CUTOFF,
                                       ptr(t.ids), ptr(t.gt), NGRAM_SLOTS, ORDER, BOS, ALPHA, BETA,
                                       ptr(buf), ptr(buf[1]), ptr(lens), ptr(scores), ptr(scores[1]), ptr(t.ws), 0))


@pytest.mark.parametrize("Tc", [0, 3])
def test_stream_entry_gets_the_headers_arguments(rec, Tc):
    from deepspeech.pytorch_amd import ops
    t = CharCase()
    h = ops.BeamStreamHandle(state=t.state, N=N, B=B, max_frames=MAX_FRAMES, C=C, blank=BLANK, top_n=TOP_N, cutoff_prob=CUTOFF,
                             lm=t.lm, hot=None, flags=5, device=torch.device("cpu"))
    if Tc == 0:
        buf, lens, scores = ops._beam_outputs(N, B, ROW_STRIDE, "cpu")
        ops._beam_stream_launch(h, None, 0, None, buf, lens, scores, ROW_STRIDE, B)
        head = (0, 0, 0, N, 0, C, 0, BLANK, B, TOP_N, CUTOFF)
        out = (ptr(buf), ptr(buf[1]), ROW_STRIDE, B, ptr(lens), ptr(scores))
        acoustic, ws = ptr(scores[1]), 0
    else:
        ops._beam_stream_launch(h, t.probs, Tc, t.sz, None, None, None, None, 0)
        head = (ptr(t.probs), (T + 1) * C, C, N, Tc, C, ptr(t.sz), BLANK, B, TOP_N, CUTOFF)
        out = (0, 0, 0, 0, 0, 0)
        acoustic, ws = 0, AnyPointer()
    # ..., float cutoff_prob, const int* cid, const void* ngram_table, long ngram_slots, int order, int bos, float alpha,
    # float beta, void* state, int max_frames, int* tokens, int* offsets, long row_stride, int out_ranks, int* lens, float* scores,
    # float* acoustic, void* ws, ds2_stream_t stream
    check(rec, "ds2_beam_stream_feed_clm", head + (ptr(t.ids), ptr(t.gt), NGRAM_SLOTS, ORDER, BOS, ALPHA, BETA)
          + (ptr(t.state), MAX_FRAMES) + out + (acoustic, ws, 0))


def test_grid_entry_gets_the_headers_arguments(rec, monkeypatch):
    from deepspeech.pytorch_amd import ops
    t = CharCase()
    held = {}

    def weights(name, w, dev):
        held[name] = torch.as_tensor(w, dtype=torch.float32)
        return held[name]

    monkeypatch.setattr(ops, "_beam_clm_checks", lambda *a: (B, TOP_N))           # they ask for device tensors
    monkeypatch.setattr(ops, "_weights", weights)

    class OnDevice(torch.Tensor):
        is_cuda = True

    alphas, betas = [0.25, 1.5, 2.0], [3.0, 0.125, 0.5]
    toks, offs, lens, scores, acoustic = ops.beam_decode_clm_grid(t.probs.as_subclass(OnDevice), t.sz, BLANK, B, TOP_N, CUTOFF, t.ids,
                                                                  t.gt, ORDER, BOS, alphas, betas)
    assert toks.shape == (3, N, T) and scores.shape == (3, N)
    assert held["alphas"].tolist() == alphas and held["betas"].tolist() == betas
    # ..., float cutoff_prob, const int* cid, const void* ngram_table, long ngram_slots, int order, int bos, int G,
    # const float* alphas, const float* betas, int* tokens, int* offsets, int* lens, float* scores, float* acoustic, void* ws,
    # ds2_stream_t stream
    check(rec, "ds2_beam_decode_clm_grid", (ptr(t.probs), (T + 1) * C, C, N, T, C, ptr(t.sz), BLANK, B, TOP_N, CUTOFF,
                                            ptr(t.ids), ptr(t.gt), NGRAM_SLOTS, ORDER, BOS, 3, ptr(held["alphas"]), ptr(held["betas"]),
                                            ptr(toks), ptr(offs), ptr(lens), ptr(scores), ptr(acoustic), AnyPointer(), 0))


def _declarations():
    """{name: number of arguments} of the header's ds2_beam_*clm* prototypes"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|long)\s+(ds2_beam_\w*clm\w*)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [a.strip() for a in m.group(2).split(",")]
    return out


def test_every_clm_declaration_has_one_ctypes_type_per_argument(lib):
    from deepspeech.pytorch_amd import _lib
    decl = _declarations()
    assert set(decl) == {"ds2_beam_decode_clm", "ds2_beam_stream_feed_clm", "ds2_beam_decode_clm_grid"}
    kinds = {_lib.C.c_void_p: "pointer", _lib.C.c_int: "int", _lib.C.c_long: "long", _lib.C.c_float: "float"}
    for name, args in decl.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is _lib.C.c_int and len(argtypes) == len(args), name
        for a, ct in zip(args, argtypes):
            want = "pointer" if "*" in a or a.startswith("ds2_stream_t") else a.split()[0]
            assert kinds[ct] == want, (name, a, ct)
        assert getattr(lib, name).argtypes == argtypes


def test_stream_size_queries_know_the_character_flag_word(lib):
    for flags in (4, 6, 7, 8, -1):
        assert lib.ds2_beam_stream_bytes(3, 16, 50, flags) == 0 and lib.ds2_beam_stream_state_stride(16, flags) == 0
    assert lib.ds2_beam_stream_bytes(3, 16, 50, 5) == lib.ds2_beam_stream_bytes(3, 16, 50, 1) > 0
    assert lib.ds2_beam_stream_state_stride(16, 5) == lib.ds2_beam_stream_state_stride(16, 1) > 0
    assert lib.ds2_beam_stream_state_stride(16, 5) >= 16 + 68 * 16
    for flags in (0, 1, 2, 3):
        assert lib.ds2_beam_stream_bytes(3, 16, 50, flags) > 0
