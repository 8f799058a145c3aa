"""Host-side checks of the streaming decoders' C ABI: the size queries of the resumable beam search (host-only, no GPU needed)
and the declared signatures."""
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ds2_beam_stream_bytes", "ds2_beam_stream_ws_bytes", "ds2_beam_stream_state_stride", "ds2_beam_stream_reset",
         "ds2_beam_stream_feed", "ds2_beam_stream_feed_lm", "ds2_greedy_stream_feed"]


@pytest.fixture(scope="module")
def lib():
    from deepspeech.pytorch_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_signatures_are_declared_exported_and_match_the_header(lib):
    from deepspeech.pytorch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ds2hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name     # one ctypes type per declared argument
    assert _lib.SIGNATURES["ds2_beam_stream_bytes"][0] is _lib.SIGNATURES["ds2_beam_stream_ws_bytes"][0] is _lib.C.c_long


def test_size_queries_are_zero_for_non_positive_arguments(lib):
    for bad in (0, -1):
        assert lib.ds2_beam_stream_bytes(bad, 16, 100, 0) == 0 and lib.ds2_beam_stream_bytes(3, bad, 100, 1) == 0
        assert lib.ds2_beam_stream_bytes(3, 16, bad, 0) == 0
        assert lib.ds2_beam_stream_ws_bytes(bad, 10) == 0 and lib.ds2_beam_stream_ws_bytes(3, bad) == 0
        assert lib.ds2_beam_stream_state_stride(bad, 0) == 0 and lib.ds2_beam_stream_state_stride(bad, 1) == 0


def test_state_stride_is_the_aligned_state_of_one_stream(lib):
    """the header's layout: 16 bytes + 32 a beam (+ 36 with an LM), 256-byte aligned; one more stream adds one stride besides pools"""
    for b in (1, 4, 7, 16, 100, 256):
        for lm in (0, 1):
            v = lib.ds2_beam_stream_state_stride(b, lm)
            assert v % 256 == 0 and 0 <= v - (16 + b * (32 + 36 * lm)) < 256
            pools = lambda n: 3 * ((n * 2 * b * 4 + 255) // 256 * 256)           # max_frames = 1: [n][2][b] int32, three arrays
            assert lib.ds2_beam_stream_bytes(3, b, 1, lm) - pools(3) == 3 * v


def test_size_queries_are_aligned_and_grow_in_every_argument(lib):
    Ns, Bs, Fs = (1, 2, 3, 64), (1, 4, 16, 100, 256), (1, 4, 100, 6000, 100000)
    raw = lambda n, b, f, lm: n * (16 + b * (32 + 36 * lm)) + 12 * n * (f + 1) * b   # the bytes in use
    size = {k: lib.ds2_beam_stream_bytes(*k) for k in itertools.product(Ns, Bs, Fs, (0, 1))}
    for (n, b, f, lm), v in size.items():
        assert v > 0 and v % 256 == 0
        # the state of every stream, and the node pool [N][max_frames + 1][B] x (parent, label, frame): 12 * B bytes a frame
        assert raw(n, b, f, lm) <= v <= raw(n, b, f, lm) + 255 * n + 3 * 255
    for axis, values in enumerate((Ns, Bs, Fs, (0, 1))):
        for k, v in size.items():
            i = values.index(k[axis])
            if i + 1 < len(values):
                bigger = k[:axis] + (values[i + 1],) + k[axis + 1:]
                assert size[bigger] >= v, (k, bigger)
                if raw(*bigger) - raw(*k) > 255 * k[0] + 3 * 255:             # more than the alignment slack (states, three pools)
                    assert size[bigger] > v, (k, bigger)
    assert lib.ds2_beam_stream_bytes(3, 16, 6000, 0) > lib.ds2_beam_stream_bytes(3, 16, 100, 0) + 12 * 3 * 16 * 5000
    ws = {(n, t): lib.ds2_beam_stream_ws_bytes(n, t) for n in Ns for t in (1, 2, 7, 100, 1000)}
    for (n, t), v in ws.items():
        assert v % 256 == 0 and v >= n * t * (4 + 2 * 64 * 4)                 # count + 64 x (class, log p) per frame
        assert all(ws[k] >= v for k in ws if k[0] >= n and k[1] >= t)
        assert all(ws[k] > v for k in ws if k[0] > n and k[1] > t)
    # the per-feed workspace knows nothing of the frames consumed or of the beam width: only of the chunk
    assert lib.ds2_beam_stream_ws_bytes(3, 100) < lib.ds2_beam_ws_bytes(3, 100, 16)
