"""Host-side check of how ops.py marshals the beam search's C calls: for each of the eight entries (one-shot and resumable;
plain, language model, hot words, both) the launch-level functions are run on CPU tensors with ops.call recorded, and the
recorded arguments must be the ones include/ds2hip.h declares, in its order.  Every table has its own slot count and alpha,
beta and oov_logp differ, so a swapped pair shows.  No GPU needed."""
import ctypes

import pytest
import torch

N, T, C, B = 2, 3, 5, 4
BLANK, TOP_N, CUTOFF, SPACE, ORDER, BOS, ALPHA, BETA, OOV = 0, 6, 0.75, 1, 3, 7, 1.25, 0.5, -11.5
WORD_SLOTS, NGRAM_SLOTS, HOT_SLOTS = 8, 16, 4
MAX_FRAMES, ROW_STRIDE = 9, 11


@pytest.fixture(scope="module")
def lib():
    from deepspeech.pytorch_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


class Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, name, *args):
        self.calls.append((name, args))
        return 0


@pytest.fixture
def rec(lib, monkeypatch):
    from deepspeech.pytorch_amd import ops
    r = Recorder()
    monkeypatch.setattr(ops, "call", r)
    monkeypatch.setattr(ops, "query", lambda name, *args: 256)
    monkeypatch.setattr(ops, "P", lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr()))
    monkeypatch.setattr(ops, "S", lambda: ctypes.c_void_p(0))
    return r


class Case:
    """the tensors of one case; ptr(t) is what the C call must receive for t"""

    def __init__(self):
        self.probs = torch.rand(N, T + 1, C)[:, :T]             # stride_n = (T + 1) * C: not what a contiguous chunk has
        self.sz = torch.tensor([3, 2], dtype=torch.int32)
        self.wt = torch.zeros((WORD_SLOTS, 2), dtype=torch.int64)
        self.gt = torch.zeros((NGRAM_SLOTS, 2), dtype=torch.int64)
        self.ht = torch.zeros((HOT_SLOTS, 2), dtype=torch.int64)
        self.ws = torch.zeros(256, dtype=torch.uint8)
        self.state = torch.zeros(512, dtype=torch.uint8)
        self.lm = dict(space=SPACE, word_table=self.wt, ngram_table=self.gt, order=ORDER, bos=BOS, alpha=ALPHA, beta=BETA,
                       lexicon=True)
        self.hot = dict(space=SPACE, table=self.ht, oov_logp=OOV)


class AnyPointer:
    """equal to every non-null pointer: the workspace that _beam_stream_launch allocates itself"""

    def __eq__(self, other):
        return isinstance(other, int) and other != 0


def ptr(t):
    return t.data_ptr()


def plain_value(a):
    return (a.value or 0) if isinstance(a, ctypes.c_void_p) else a


def check(rec, name, expected):
    from deepspeech.pytorch_amd import _lib
    assert len(rec.calls) == 1
    got_name, args = rec.calls[0]
    assert got_name == name
    argtypes = _lib.SIGNATURES[name][1]
    assert len(args) == len(argtypes)
    for argtype, arg in zip(argtypes, args):
        argtype.from_param(arg)                                 # raises where ctypes would refuse the argument
    got = tuple(plain_value(a) for a in args)
    assert len(got) == len(expected)
    for i, (g, e) in enumerate(zip(got, expected)):
        assert e == g and (isinstance(e, AnyPointer) or type(e) is type(g)), (name, i, g, e)


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("with_hot", [False, True])
def test_one_shot_entries_get_the_headers_arguments(rec, with_lm, with_hot):
    from deepspeech.pytorch_amd import ops
    t = Case()
    buf, lens, scores = ops._beam_outputs(N, B, T, "cpu")
    assert buf.shape == (2, N, B, T) and lens.shape == (N, B) and scores.shape == (2, N, B)
    ops._beam_launch(t.probs, t.sz, BLANK, B, TOP_N, CUTOFF, t.lm if with_lm else None, t.hot if with_hot else None, buf, lens,
                     scores, t.ws)
    # const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank, int B, int cutoff_top_n,
    # float cutoff_prob
    head = (ptr(t.probs), (T + 1) * C, C, N, T, C, ptr(t.sz), BLANK, B, TOP_N, CUTOFF)
    tokens, offsets, sc, ac = ptr(buf), ptr(buf[1]), ptr(scores), ptr(scores[1])
    if not with_lm and not with_hot:
        # int* tokens, int* offsets, int* lens, float* scores, void* ws, ds2_stream_t stream
        check(rec, "ds2_beam_decode", head + (tokens, offsets, ptr(lens), sc, ptr(t.ws), 0))
    elif with_lm and not with_hot:
        # int space, const void* word_table, long word_slots, const void* ngram_table, long ngram_slots, int order, int bos,
        # float alpha, float beta, int lexicon, int* tokens, int* offsets, int* lens, float* scores, float* acoustic, void* ws,
        # ds2_stream_t stream
        check(rec, "ds2_beam_decode_lm", head + (SPACE, ptr(t.wt), WORD_SLOTS, ptr(t.gt), NGRAM_SLOTS, ORDER, BOS, ALPHA, BETA, 1,
                                                 tokens, offsets, ptr(lens), sc, ac, ptr(t.ws), 0))
    elif with_hot and not with_lm:
        # int space, const void* hot_table, long hot_slots, int* tokens, int* offsets, int* lens, float* scores, float* acoustic,
        # void* ws, ds2_stream_t stream
        check(rec, "ds2_beam_decode_hot", head + (SPACE, ptr(t.ht), HOT_SLOTS, tokens, offsets, ptr(lens), sc, ac, ptr(t.ws), 0))
    else:
        # int space, const void* word_table, long word_slots, const void* ngram_table, long ngram_slots, int order, int bos,
        # float alpha, float beta, int lexicon, const void* hot_table, long hot_slots, float hot_oov_logp, int* tokens,
        # int* offsets, int* lens, float* scores, float* acoustic, void* ws, ds2_stream_t stream
        check(rec, "ds2_beam_decode_lm_hot", head + (SPACE, ptr(t.wt), WORD_SLOTS, ptr(t.gt), NGRAM_SLOTS, ORDER, BOS, ALPHA, BETA,
                                                     1, ptr(t.ht), HOT_SLOTS, OOV, tokens, offsets, ptr(lens), sc, ac, ptr(t.ws), 0))


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("with_hot", [False, True])
@pytest.mark.parametrize("Tc", [0, 3])
def test_stream_entries_get_the_headers_arguments(rec, with_lm, with_hot, Tc):
    """Tc == 0 with the output stage (no chunk, no sizes, no workspace); Tc == 3 without it (no outputs)"""
    from deepspeech.pytorch_amd import ops
    t = Case()
    h = ops.BeamStreamHandle(state=t.state, N=N, B=B, max_frames=MAX_FRAMES, C=C, blank=BLANK, top_n=TOP_N, cutoff_prob=CUTOFF,
                             lm=t.lm if with_lm else None, hot=t.hot if with_hot else None, flags=with_lm + 2 * with_hot,
                             device=torch.device("cpu"))
    if Tc == 0:
        buf, lens, scores = ops._beam_outputs(N, B, ROW_STRIDE, "cpu")
        ops._beam_stream_launch(h, None, 0, None, buf, lens, scores, ROW_STRIDE, B)
        # const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, ...
        head = (0, 0, 0, N, 0, C, 0, BLANK, B, TOP_N, CUTOFF)
        # int* tokens, int* offsets, long row_stride, int out_ranks, int* lens, float* scores
        out = (ptr(buf), ptr(buf[1]), ROW_STRIDE, B, ptr(lens), ptr(scores))
        acoustic, ws = ptr(scores[1]), 0
    else:
        ops._beam_stream_launch(h, t.probs, Tc, t.sz, None, None, None, None, 0)
        head = (ptr(t.probs), (T + 1) * C, C, N, Tc, C, ptr(t.sz), BLANK, B, TOP_N, CUTOFF)
        out = (0, 0, 0, 0, 0, 0)
        acoustic, ws = 0, AnyPointer()
    # void* state, int max_frames
    state = (ptr(t.state), MAX_FRAMES)
    if not with_lm and not with_hot:
        # ..., float cutoff_prob, void* state, int max_frames, <out>, void* ws, ds2_stream_t stream
        check(rec, "ds2_beam_stream_feed", head + state + out + (ws, 0))
    elif with_lm and not with_hot:
        # ..., int space, const void* word_table, long word_slots, const void* ngram_table, long ngram_slots, int order, int bos,
        # float alpha, float beta, int lexicon, void* state, int max_frames, <out>, float* acoustic, void* ws, ds2_stream_t stream
        check(rec, "ds2_beam_stream_feed_lm", head + (SPACE, ptr(t.wt), WORD_SLOTS, ptr(t.gt), NGRAM_SLOTS, ORDER, BOS, ALPHA, BETA, 1)
              + state + out + (acoustic, ws, 0))
    elif with_hot and not with_lm:
        # ..., int space, const void* hot_table, long hot_slots, void* state, int max_frames, <out>, float* acoustic, void* ws,
        # ds2_stream_t stream
        check(rec, "ds2_beam_stream_feed_hot", head + (SPACE, ptr(t.ht), HOT_SLOTS) + state + out + (acoustic, ws, 0))
    else:
        # ..., int space, const void* word_table, long word_slots, const void* ngram_table, long ngram_slots, int order, int bos,
        # float alpha, float beta, int lexicon, const void* hot_table, long hot_slots, float hot_oov_logp, void* state,
        # int max_frames, <out>, float* acoustic, void* ws, ds2_stream_t stream
        check(rec, "ds2_beam_stream_feed_lm_hot", head + (SPACE, ptr(t.wt), WORD_SLOTS, ptr(t.gt), NGRAM_SLOTS, ORDER, BOS, ALPHA,
                                                          BETA, 1, ptr(t.ht), HOT_SLOTS, OOV) + state + out + (acoustic, ws, 0))
