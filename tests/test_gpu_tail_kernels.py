"""Two small kernels of the training step's tail, bit for bit: the recurrent layers' bias gradients (ds2_rnn_bias_grads, which issues
its per-sample loads in batches but adds them in sample order) and the AdamW / SGD update of the column-permuted rnns.0.weight_ih
with its two bf16 layouts (k_opt_matrix_perm_rows against k_opt_matrix_perm, the kernel it replaced on that matrix)."""
import ctypes as C
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("kind", ["gru", "lstm", "rnn"])
@pytest.mark.parametrize("N", [1, 7, 8, 9, 32])
@pytest.mark.parametrize("H", [32, 1024])
@pytest.mark.parametrize("D", [1, 2])
def test_rnn_bias_grads_add_the_samples_in_index_order(kind, N, H, D):
    """bias_ih.grad / bias_hh.grad = the per-sample sums of the BPTT sweep added n = 0 .. N-1 in fp32: the same bits as a torch loop
    over the samples (N = 7 / 8 / 9 straddle the batch of eight loads, 32 is four whole batches)."""
    from deepspeech.pytorch_amd import ops
    G = ops.GATES[kind]
    NB = 4 if kind == "gru" else G
    g = torch.Generator().manual_seed(1000 * N + H + D)
    bacc = (torch.randn((D, N, NB * H), generator=g) * torch.logspace(-3, 3, NB * H)).to(DEV)
    dbih, dbhh = ops.rnn_bias_grads(kind, bacc, D, N, H)
    s = torch.zeros((D, NB * H), dtype=torch.float32, device=DEV)
    for n in range(N):
        s = s + bacc[:, n]
    s = s.reshape(D, NB, H)
    want_ih = s[:, :G].reshape(D * G * H)
    want_hh = (s[:, [0, 1, 3]] if kind == "gru" else s).reshape(D, G * H)      # GRU: the hidden side's n slot is dq = dn * r
    assert torch.equal(dbih, want_ih)
    assert torch.equal(dbhh, want_hh)


PERM_CASES = [(96, 0, False), (96, 0, True), (96, 1, False), (3072, 0, True)]
PERM_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "opt_matrix_perm_parent.json")


def _opt_case(R, Cc, seed):
    g = torch.Generator().manual_seed(seed)
    w, gr = torch.randn((R, Cc), generator=g), torch.randn((R, Cc), generator=g)
    m0, v0 = torch.randn((R, Cc), generator=g) * 0.1, torch.rand((R, Cc), generator=g) * 0.01
    return [t.to(DEV) for t in (w, gr, m0, v0)]


def run_perm_update(R, mode, clip, ldd_pad=0):
    """ds2_opt_matrix on a seeded rnns.0.weight_ih-shaped case (32 channels x 41 features = 1 312 columns, permuted c*41+f -> f*32+c,
    32 zero pad columns).  Returns (weights, first moment, second moment, bf16 copy [R][Cout + ldd_pad], bf16 transpose)."""
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd._lib import call
    Cc, perm_c, perm_f, Cout = 1312, 32, 41, 1344
    hp = (C.c_float * 7)(1 - 1e-3, 0.1, 0.999, 0.001, 0.0316, 1e-8, -0.015) if mode == 0 else (C.c_float * 7)(1e-4, 0.9, 0, 0, 0, 0, -0.01)
    clip_t = torch.tensor([3.0, 0.37], dtype=torch.float32, device=DEV) if clip else None
    a = _opt_case(R, Cc, seed=R + mode)
    w0 = a[0].clone()
    dst = torch.full((R, Cout + ldd_pad), 7.0, dtype=torch.bfloat16, device=DEV)
    dstT = torch.full((Cout, R), 7.0, dtype=torch.bfloat16, device=DEV)
    call("ds2_opt_matrix", mode, ops.P(a[0]), ops.P(a[1]), ops.P(a[2]), ops.P(a[3]), R, Cc, perm_c, perm_f, Cout, ops.P(dst), Cout + ldd_pad,
         ops.P(dstT), R, hp, 0, ops.P(clip_t), ops.S())
    torch.cuda.synchronize()
    assert not torch.equal(a[0], w0)          # the update happened
    return a[0], a[2], a[3], dst, dstT


def digests(tensors):
    return [hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest() for t in tensors]


@pytest.mark.parametrize("R,mode,clip", PERM_CASES)
def test_permuted_matrix_update_keeps_the_bits_of_the_kernel_it_replaced(R, mode, clip):
    """rnns.0.weight_ih at its real column count: one 32-row gate tile per gate (96 rows) and the cfg3 matrix (3 072 rows).  Updated
    weights, both moments, the bf16 copy and the bf16 transpose of k_opt_matrix_perm_rows are compared (a) with the SHA-256 digests of
    what the parent commit's k_opt_matrix_perm wrote for the same seeded inputs, recorded on an MI355X from the parent's build
    (tests/golden/opt_matrix_perm_parent.json), and (b) with that kernel as it still is in the library, which ds2_opt_matrix takes
    when the bf16 copy's row stride is not a multiple of 8 elements (here: Cout + 4); (b)'s own digests must be the recorded ones
    too, so the comparison cannot silently become new against new."""
    Cc, Cout = 1312, 1344
    golden = json.load(open(PERM_GOLDEN))["%d_%d_%d" % (R, mode, int(clip))]
    new = run_perm_update(R, mode, clip)
    old = run_perm_update(R, mode, clip, ldd_pad=4)
    assert digests(new) == golden
    assert digests(old[:3] + (old[3][:, :Cout], old[4])) == golden
    assert not bool(new[3][:, Cc:].any()) and not bool(new[4][Cc:].any())          # the pad columns are zero
    assert bool((old[3][:, Cout:] == 7.0).all())                                   # and nothing is written past them
