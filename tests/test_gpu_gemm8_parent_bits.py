"""The 256x256 phase-split GEMM (csrc/ds2_gemm8.hip) keeps the bits of the commit before its first-round start offsets: neither
when a tile starts nor in which phase a fragment is read changes which MFMA adds what in which order.  A seeded set of small launches
-- NT and grouped TN with 1, 2, 3, 4 and 7 K-tiles, ragged TN K (40, 100, 333), edge tiles in M and N, bias, both output types, the
two-buffer A operand, row lists (T' x N = 37 x 8 and 151 x 32) and the mixed launch -- is compared with the SHA-256 digests of what
that commit's build wrote for the same inputs, recorded on an MI355X (tests/golden/gemm8_parent.json).

    python tests/test_gpu_gemm8_parent_bits.py OUT.json        # records the digests of the build that is importable"""
import hashlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm8_parent.json")


def _rand(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1).to(DEV).to(torch.bfloat16)


def _frame_list(Tp, N, seed):
    import numpy as np
    rs = np.random.RandomState(seed)
    lens = rs.randint(max(1, Tp // 3), Tp + 1, N).astype(np.int32)
    lens[rs.randint(N)] = Tp
    rows = np.flatnonzero(np.arange(Tp)[:, None] < lens[None, :]).astype(np.int32)
    return torch.from_numpy(lens).to(DEV), torch.from_numpy(rows).to(DEV)


def digests(tensors):
    torch.cuda.synchronize()
    return [hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest() for t in tensors]


def _nt(M, N, K, f32, bias):
    from deepspeech.pytorch_amd import ops
    A, B = _rand((M, K), 100 + K), _rand((N, K), 200 + K)
    bv = torch.linspace(-1, 1, N, device=DEV) if bias else None
    return [ops.gemm8_nt(A, B, bias=bv, out_dtype=torch.float32 if f32 else None)]


def _nt_strided():
    from deepspeech.pytorch_amd import ops
    Aw, Bw = _rand((700, 512), 3), _rand((300, 384), 4)
    return [ops.gemm8_nt(Aw[:, 128:384], Bw[:, 64:320], M=700, N=300, K=256, lda=512, ldb=384)]


def _nt_rows(Tp, N, K, Nc, f32, bias):
    from deepspeech.pytorch_amd import ops, _lib
    R = Tp * N
    _, rows = _frame_list(Tp, N, 41)
    A, B = _rand((R, K), 42), _rand((Nc, K), 43)
    bv = torch.linspace(-1, 1, Nc, device=DEV) if bias else None
    out = torch.zeros((R, Nc), dtype=torch.float32 if f32 else torch.bfloat16, device=DEV)       # unlisted rows stay zero
    _lib.call("ds2_gemm8_nt_rows", ops.P(A), ops.P(B), ops.P(out), ops.PF(bv), R, Nc, K, K, K, Nc, 1 if f32 else 0, ops.P(rows), rows.numel(),
              ops.S())
    return [out]


def _tn(K):
    """three products in one launch: edge tiles in M and N, the two-buffer A operand, column windows of wider matrices"""
    from deepspeech.pytorch_amd import ops
    At0, Bt0 = _rand((K, 520), 5), _rand((K, 264), 6)
    At1, At1b, Bt1 = _rand((K, 768), 7), _rand((K, 256), 8), _rand((K, 256), 9)
    At2w, Bt2w = _rand((K, 1024), 10), _rand((K, 640), 11)
    probs = [dict(At=At0, Bt=Bt0, M=520, N=264, lda=520, ldb=264),
             dict(At=At1, At2=At1b, lda2=256, m_split=512, Bt=Bt1, M=768, N=256, lda=768, ldb=256),
             dict(At=At2w[:, 256:], Bt=Bt2w[:, 128:], M=768, N=512, lda=1024, ldb=640)]
    return ops.gemm8_tn_grouped(probs, K)


def _layer_operands(R, H, seed):
    dG, X, Hp, dQ = _rand((R, 3 * H), seed), _rand((R, H + 64), seed + 1)[:, :H], _rand((R, H), seed + 2), _rand((R, H), seed + 3)
    W = _rand((H, 3 * H), seed + 4)
    probs = [dict(At=dG, Bt=X, M=3 * H, N=H, lda=3 * H, ldb=X.stride(0)),
             dict(At=dG, At2=dQ, lda2=H, m_split=2 * H, Bt=Hp, M=3 * H, N=H, lda=3 * H, ldb=H)]
    return probs, dG, W


def _mixed(R):
    """the weight-gradient problems and the NT dX product in one launch (no row list)"""
    from deepspeech.pytorch_amd import ops
    probs, dG, W = _layer_operands(R, 512, 60)
    outs, dx = ops.gemm8_tn_grouped(probs, R, dx=(dG, W))
    return outs + [dx]


def _rows_tn_and_mixed(Tp, N):
    """grouped TN over a row list, then the mixed launch over the same list (dX: listed rows, zeros elsewhere)"""
    from deepspeech.pytorch_amd import ops
    R = Tp * N
    lens, rows = _frame_list(Tp, N, 51)
    probs, dG, W = _layer_operands(R, 512, 70)
    outs = ops.gemm8_tn_grouped(probs, R, rows=rows)
    outs_m, dx = ops.gemm8_tn_grouped(probs, R, dx=(dG, W), rows=rows, zero_pad=(lens, Tp, N))
    return outs + outs_m + [dx]


CASES = {}
for _M, _N, _K, _f32, _bias in [(256, 256, 64, True, False), (300, 520, 128, False, True), (1000, 264, 192, True, True),
                                (520, 300, 256, False, False), (300, 264, 448, False, True), (264, 520, 448, True, False)]:
    CASES["nt_%d_%d_%d_%d_%d" % (_M, _N, _K, _f32, _bias)] = (_nt, (_M, _N, _K, _f32, _bias))
CASES["nt_strided"] = (_nt_strided, ())
CASES["nt_rows_37_8"] = (_nt_rows, (37, 8, 64, 264, True, True))
CASES["nt_rows_151_32"] = (_nt_rows, (151, 32, 320, 1344, False, True))
for _K in (64, 128, 192, 256, 448, 40, 100, 333):
    CASES["tn_%d" % _K] = (_tn, (_K,))
CASES["mixed_1040"] = (_mixed, (1040,))          # ragged K for the TN problems (16 K-tiles + 16 rows)
CASES["mixed_128"] = (_mixed, (128,))            # two K-tiles
CASES["rows_tn_mixed_37_8"] = (_rows_tn_and_mixed, (37, 8))
CASES["rows_tn_mixed_151_32"] = (_rows_tn_and_mixed, (151, 32))


@pytest.mark.parametrize("name", sorted(CASES))
def test_gemm8_keeps_the_bits_of_the_parent_build(name):
    golden = json.load(open(GOLDEN))
    fn, args = CASES[name]
    first = digests(fn(*args))
    assert first == golden[name]
    assert digests(fn(*args)) == first            # a second launch: nothing carried over


def test_golden_file_covers_exactly_these_cases():
    assert sorted(json.load(open(GOLDEN))) == sorted(CASES)


if __name__ == "__main__":
    rec = {name: digests(fn(*args)) for name, (fn, args) in sorted(CASES.items())}
    again = {name: digests(fn(*args)) for name, (fn, args) in sorted(CASES.items())}
    assert rec == again, "the recording build is not deterministic"
    json.dump(rec, open(sys.argv[1], "w"), indent=1, sort_keys=True)
    print("recorded %d cases, %d tensors" % (len(rec), sum(len(v) for v in rec.values())))
