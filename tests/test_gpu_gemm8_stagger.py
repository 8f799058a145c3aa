"""First-round start offsets of the NT launches of csrc/ds2_gemm8.hip (g8_stagger_wait): the workgroups that open the CUs wait
id * span / CUs before their first tile.  The wait decides WHEN a tile runs, never what it computes: every result with a forced span
-- a short one, the clamp value, and a request far beyond the clamp -- equals the span-0 result bit for bit, twice in a row."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rand(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1).to(DEV).to(torch.bfloat16)


def _clamp():
    from deepspeech.pytorch_amd._lib import query
    return query("ds2_gemm8_stagger_plan", -1, 0, 0)


@pytest.mark.parametrize("M,N,K,f32,bias", [
    (256, 256, 64, True, False),          # one tile: only workgroup 0, whose wait is zero
    (300, 520, 128, False, True),         # edge tiles in M and N: six workgroups with different waits
    (4352, 4096, 64, False, False),       # 272 tiles: a whole round of 256 CUs and a 16-tile tail that inherits its phase
])
def test_forced_span_does_not_change_the_result(M, N, K, f32, bias):
    from deepspeech.pytorch_amd import ops
    A, B = _rand((M, K), 1), _rand((N, K), 2)
    bv = torch.linspace(-1, 1, N, device=DEV) if bias else None
    od = torch.float32 if f32 else None
    want = ops.gemm8_nt(A, B, bias=bv, out_dtype=od, stagger_us=0)
    assert torch.equal(want, ops.gemm8_nt(A, B, bias=bv, out_dtype=od))            # the policy's span
    for span in (25, _clamp(), 10 ** 9):
        for rep in range(2):
            got = ops.gemm8_nt(A, B, bias=bv, out_dtype=od, stagger_us=span)
            assert torch.equal(got, want), (span, rep)


def test_forced_span_with_a_row_list():
    """151 x 32 frames, about two thirds listed: 13 x 6 tiles; unlisted rows of the output stay untouched under every span."""
    import numpy as np
    from deepspeech.pytorch_amd import ops, _lib
    Tp, Nb, K, Nc = 151, 32, 320, 1344
    R = Tp * Nb
    rs = np.random.RandomState(7)
    lens = rs.randint(Tp // 3, Tp + 1, Nb)
    rows = torch.from_numpy(np.flatnonzero(np.arange(Tp)[:, None] < lens[None, :]).astype(np.int32)).to(DEV)
    A, B = _rand((R, K), 3), _rand((Nc, K), 4)
    bv = torch.linspace(-1, 1, Nc, device=DEV)

    def run(span):
        out = torch.full((R, Nc), 7.0, dtype=torch.bfloat16, device=DEV)
        _lib.call("ds2_gemm8_nt_rows_stagger", ops.P(A), ops.P(B), ops.P(out), ops.PF(bv), R, Nc, K, K, K, Nc, 0, ops.P(rows), rows.numel(),
                  span, ops.S())
        return out
    want = run(0)
    listed = torch.zeros(R, dtype=torch.bool, device=DEV)
    listed[rows.long()] = True
    assert bool((want[~listed] == 7.0).all()) and not bool((want[listed] == 7.0).all())
    assert torch.equal(want[listed], ops.gemm8_nt(A, B, bias=bv)[listed])
    for span in (-1, 25, _clamp()):
        for rep in range(2):
            assert torch.equal(run(span), want), (span, rep)
    assert torch.equal(ops.gemm8_nt(A, B, bias=bv, rows=rows, stagger_us=25)[listed], want[listed])
