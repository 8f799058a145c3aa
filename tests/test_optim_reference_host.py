"""The float64 optimizer reference (tests/optim_reference.py) against torch.optim on the CPU, with the measurement that sets the
tolerance of tests/test_gpu_optim_routes.py, and the routing table of ds2_opt_matrix (ds2_opt_matrix_route, host only) for every
matrix case of that file.  No device."""
import numpy as np
import pytest
import torch

import optim_reference as O

ADAMW = dict(lr=1.5e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
SGD = dict(lr=3e-2, momentum=0.9, weight_decay=1e-3)


@pytest.fixture(scope="module")
def lib():
    from deepspeech.pytorch_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def _torch_clip(params, max_norm):
    """clip_grad_norm_ on the CPU.  Returns (its total norm, the fp32 coefficient it multiplied the gradients by)."""
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    return float(total), float(torch.clamp(max_norm / (total + 1e-6), max=1.0))


def _torch_run(mode, clip, inject, worst, eps=None):
    """Three steps from fresh state, or (inject) one step from random non-zero moments at step count 2; every step against
    O.update() from torch's own fp32 state before it.  Folds the distances into `worst`."""
    ws = O.tensors(1 + mode)
    params = [torch.nn.Parameter(torch.from_numpy(w.copy())) for w in ws]
    adamw = dict(ADAMW, eps=eps) if eps else ADAMW
    opt = torch.optim.AdamW(params, foreach=False, **adamw) if mode == 0 else torch.optim.SGD(params, nesterov=True, foreach=False, **SGD)
    done = 0
    if inject:
        rs = np.random.RandomState(77 + mode)
        for p in params:
            m0 = torch.from_numpy(O.signed(rs, p.shape, 0.1))
            if mode == 0:
                v0 = torch.from_numpy(np.abs(O.signed(rs, p.shape, 0.01)))
                opt.state[p].update(step=torch.tensor(2.0), exp_avg=m0, exp_avg_sq=v0)
            else:
                opt.state[p]["momentum_buffer"] = m0
        done = 2
    for step in range(1 if inject else 3):
        gs = O.tensors(10 * (1 + mode) + step)
        for p, g in zip(params, gs):
            p.grad = torch.from_numpy(g.copy())
        before = []
        for p in params:
            st = opt.state[p]
            if mode == 0:
                before.append((p.detach().clone(), st["exp_avg"].clone() if st else torch.zeros_like(p), st["exp_avg_sq"].clone() if st else torch.zeros_like(p)))
            else:
                before.append((p.detach().clone(), st["momentum_buffer"].clone() if st else torch.zeros_like(p), None))
        cs = 1.0
        if clip is not None:
            norm_ref, coef_ref = O.clip_reference(gs, clip)
            total, cs = _torch_clip(params, clip)
            assert abs(total - norm_ref) <= O.CLIP_RTOL * norm_ref
            assert abs(cs - coef_ref) <= O.CLIP_RTOL * coef_ref
        opt.step()
        done += 1
        first = int(mode == 1 and done == 1)
        hp = O.adamw_hp(step=done, **adamw) if mode == 0 else O.sgd_hp(**SGD)
        for p, g, (p0, m0, v0) in zip(params, gs, before):
            ref = O.update(mode, hp, p0, g, m0, v0, cs=cs, first=first)
            st = opt.state[p]
            d = O.distances(ref, p, st["exp_avg"] if mode == 0 else st["momentum_buffer"], st["exp_avg_sq"] if mode == 0 else None)
            for k, x in d.items():
                key = ("adamw" if mode == 0 else "sgd", k)
                if x > worst.get(key, (0.0,))[0]:
                    worst[key] = (x, "clip %s, %s step %d, %d elements" % (clip, "injected," if inject else "", done, p.numel()))


def test_reference_is_what_torch_computes_and_torch_fp32_sets_k():
    """torch.optim.AdamW / SGD(nesterov) + clip_grad_norm_ in fp32 on the CPU against the float64 reference under the per-element
    measures of optim_reference.py, at every step of every run.  The largest distance is printed: it is the K_TORCH written down in
    optim_reference.py (2.2333 where it was measured), from which the kernels' K = 2 K_TORCH follows.  Asserted: torch stays inside
    the K the kernels are held to -- the reference is the same operation -- and is not so far inside that K_TORCH overstates it
    (another build of torch may round a statement differently, so the recorded figure is not pinned digit for digit).  The
    gradients' norm is about 300: clip 0.75 scales them by ~ 0.003, clip 100 by ~ 0.35."""
    worst = {}
    for mode in (0, 1):
        for clip in (None, 0.75, 100.0):
            for inject in (False, True):
                _torch_run(mode, clip, inject, worst)
    for clip in (None, 100.0):
        for inject in (False, True):
            _torch_run(0, clip, inject, worst, eps=O.BIG_EPS)
    for key in sorted(worst):
        print("torch fp32 vs float64 reference: %-5s %s  K = %.4f  (%s)" % (key[0], key[1], worst[key][0], worst[key][1]))
    top = max(x for x, _ in worst.values())
    print("largest: %.4f; K_TORCH = %.2f, K = %.2f" % (top, O.K_TORCH, O.K))
    assert set(worst) == {("adamw", "p"), ("adamw", "m"), ("adamw", "v"), ("sgd", "p"), ("sgd", "m")}
    assert O.K == 2 * O.K_TORCH
    assert O.K_TORCH / 2 <= top <= O.K


def test_reference_measures_see_a_wrong_update():
    """The measures are not so wide that a subtly wrong update passes: m read through the v pointer, beta2 for beta1, a missing clip
    coefficient, SGD without the Nesterov term, `first` ignored -- each is far outside K."""
    rs = np.random.RandomState(5)
    p0, g, m0, v0 = O.signed(rs, 4096), O.signed(rs, 4096), O.signed(rs, 4096, 0.1), np.abs(O.signed(rs, 4096, 0.01))
    hp = O.adamw_hp(step=3, **ADAMW)
    ref = O.update(0, hp, p0, g, m0, v0, cs=0.37)
    f32 = lambda r: {k: r[k].astype(np.float32) for k in ("p", "m", "v") if r[k] is not None}
    good = f32(ref)
    assert max(O.distances(ref, **good).values()) <= 1.0                             # correctly rounded results: half an ulp
    bad = f32(O.update(0, hp, p0, g, v0, v0, cs=0.37))                               # m loaded through the v pointer
    assert O.distances(ref, **bad)["m"] > 1e3 and O.distances(ref, **bad)["p"] > 1e3
    hp2 = list(hp)
    hp2[1] = 1 - hp[2]                                                               # lerp weight from beta2
    assert O.distances(ref, **f32(O.update(0, hp2, p0, g, m0, v0, cs=0.37)))["m"] > 1e3
    assert O.distances(ref, **f32(O.update(0, hp, p0, g, m0, v0, cs=1.0)))["v"] > 1e3        # clip not applied
    hs = O.sgd_hp(**SGD)
    rs_ = O.update(1, hs, p0, g, m0, cs=0.37)
    plain = rs_["p"] - hs[6] * hs[1] * rs_["m"]                                      # p without momentum * buf in the step
    assert O.distance(plain.astype(np.float32), rs_["p"], rs_["p_scale"]) > 1e3
    r1 = O.update(1, hs, p0, g, np.full(4096, 1e30, np.float32), cs=0.37, first=1)
    assert np.array_equal(r1["m"], 0.37 * g.astype(np.float64) + hs[0] * p0.astype(np.float64))      # the old buffer is ignored
    assert O.distance(rs_["m"].astype(np.float32), r1["m"], r1["m_scale"]) > 1e3


def test_clip_and_layout_references():
    g = [np.array([3.0, 0.0], np.float32), np.array([[4.0]], np.float32)]
    assert O.clip_reference(g, 10.0) == (5.0, 1.0)
    norm, coef = O.clip_reference(g, 2.5)
    assert norm == 5.0 and coef == 2.5 / (5.0 + 1e-6)
    assert O.clip_reference([np.zeros(5, np.float32)], 1.0) == (0.0, 1.0)
    p = torch.arange(2 * 6, dtype=torch.float32).reshape(2, 6) + 0.5
    d, dT = O.layouts(p, 0, 0, 8)
    assert torch.equal(d[:, :6], p.to(torch.bfloat16)) and not d[:, 6:].any() and torch.equal(dT, d.t())
    d, dT = O.layouts(p, 2, 3, 7)                      # output column f * 2 + c <- source column c * 3 + f
    for c in range(2):
        for f in range(3):
            assert torch.equal(d[:, f * 2 + c], p[:, c * 3 + f].to(torch.bfloat16))
    assert not d[:, 6:].any() and dT.shape == (7, 2) and torch.equal(dT, d.t())


# ---- the routing table ------------------------------------------------------------------------------------------------------
BASE = 0x7F0000000000          # fake pointers: ds2_opt_matrix_route looks at their alignment only
P, G, M, V, DST, DSTT = (BASE + i * 0x10000000 for i in range(6))


def _route(lib, c, mode=0, p=P, g=G, m=M, v=V, dst=DST, dstT=DSTT, **over):
    a = dict(c, **over)
    return lib.ds2_opt_matrix_route(mode, None if p is None else p + 4 * a["p_offset"], g, m, v, a["R"], a["C"], a["perm_c"], a["perm_f"], a["Cout"], dst, a["ldd"], dstT, a["lddT"])


@pytest.mark.parametrize("c", O.MATRIX_CASES, ids=O.case_id)
def test_route_of_every_matrix_case(lib, c):
    for mode, v in ((0, V), (1, V), (1, None)):
        assert _route(lib, c, mode, v=v) == c["route"]
        assert _route(lib, c, mode, v=v, dstT=None) == c["route"]
        assert _route(lib, c, mode, v=v, dst=None) == c["route_no_dst"]
        assert _route(lib, c, mode, v=v, dst=None, dstT=None) == c["route_no_dst"]
    assert c["ldd"] > c["Cout"] and c["lddT"] == c["R"] + 8


def test_every_route_is_named():
    assert {c["route"] for c in O.MATRIX_CASES} == {O.MATRIX4, O.PERM_ROWS, O.PERM, O.GENERIC}


def test_route_limits_and_alignment(lib):
    """Where one kernel hands over to the next: the 64 KB LDS image of perm_rows, operand alignment (SGD never reads v, so v's
    alignment counts for AdamW only), the bf16 copy's row stride and base."""
    c = O._case(O.PERM_ROWS, 16, 4096, 4096, (32, 128))
    assert _route(lib, c) == O.PERM_ROWS                                              # 16 rows x 16 channels x 128 x 2 B = 65536
    assert _route(lib, O._case(O.PERM, 16, 4128, 4128, (32, 129))) == O.PERM          # 66048
    assert _route(lib, O._case(O.PERM_ROWS, 16, 8192, 8192, (8, 1024))) == O.PERM     # one block of all 8 channels: 262144
    assert _route(lib, c, ldd=4100) == O.PERM and _route(lib, c, dst=DST + 8) == O.PERM
    for mode, want in ((0, O.GENERIC), (1, O.PERM_ROWS)):
        assert _route(lib, c, mode, v=V + 4) == want
    for k in ("p", "g", "m"):
        assert _route(lib, c, **{k: BASE + 4}) == O.GENERIC
    c4 = O._case(O.MATRIX4, 48, 200)
    assert _route(lib, c4) == O.MATRIX4 and _route(lib, c4, ldd=202) == O.GENERIC and _route(lib, c4, dst=DST + 8) == O.GENERIC
    assert _route(lib, c4, Cout=208) == O.GENERIC and _route(lib, c4, 0, v=V + 8) == O.GENERIC and _route(lib, c4, 1, v=V + 8) == O.MATRIX4
    assert _route(lib, c4, ldd=202, dst=None) == O.MATRIX4                            # ldd is not looked at without a copy


def test_route_rejects_what_ds2_opt_matrix_rejects(lib):
    c = O._case(O.MATRIX4, 48, 200)
    ARG, ALIGN = -1002, -1003
    assert _route(lib, c) == 0
    assert _route(lib, c, mode=2) == ARG and _route(lib, c, mode=-1) == ARG
    for k in ("p", "g", "m"):
        assert _route(lib, c, **{k: None}) == ARG
    assert _route(lib, c, 0, v=None) == ARG and _route(lib, c, 1, v=None) == 0
    for R in (0, -16, 8, 40, 47):
        assert _route(lib, c, R=R) == ARG                                             # R % 16
    assert _route(lib, c, C=0) == ARG and _route(lib, c, Cout=199) == ARG             # Cout >= C
    assert _route(lib, c, perm_c=8, perm_f=24) == ARG and _route(lib, c, perm_c=7, perm_f=0) == ARG      # perm_c * perm_f == C
    assert _route(lib, c, perm_c=8, perm_f=25) == O.PERM_ROWS
    for lddT in (57, 60, 52):
        assert _route(lib, c, lddT=lddT) == ALIGN                                     # lddT % 8
    assert _route(lib, c, lddT=57, dstT=None) == 0
    for off in (2, 4, 8):
        assert _route(lib, c, dstT=DSTT + off) == ALIGN                               # dstT on 16 bytes
    assert _route(lib, c, R=40, lddT=57) == ARG                                       # the argument checks come first
    # ds2_opt_matrix itself returns the same codes before it launches anything (null hp is its own check)
    hp = (__import__("ctypes").c_float * 7)(*O.adamw_hp(step=1, **ADAMW))
    raw = lambda **o: lib.ds2_opt_matrix(0, P, G, M, V, o.get("R", 48), 200, 0, 0, o.get("Cout", 200), DST, 208, o.get("dstT", DSTT),
                                         o.get("lddT", 56), o.get("hp", hp), 0, None, None)
    assert raw(R=40) == 1002 and raw(Cout=199) == 1002 and raw(lddT=57) == 1003 and raw(dstT=DSTT + 8) == 1003 and raw(hp=None) == 1002
