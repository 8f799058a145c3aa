"""Every kernel route of csrc/ds2_optim.hip against the float64 reference of tests/optim_reference.py (tolerance and operands:
its docstring; no kernel of this project on the reference side).

ds2_opt_matrix: each case of optim_reference.MATRIX_CASES asserts the kernel it takes (ds2_opt_matrix_route on the real pointers)
and runs AdamW, SGD, SGD's first step over a momentum buffer of 1e30 and SGD without a v pointer; without a clip pointer, with
[x, 0.37] and with [x, 1.0] (the same bits as without); writing the bf16 copy, the transpose, neither and both.  The fp32
operands sit inside guarded buffers, the bf16 windows inside larger buffers of 7.0 with ldd > Cout and lddT = R + 8: guards, g, an
unused v and everything outside the windows keep their bits, and the layouts are, bit for bit, those of the updated matrix.
ds2_opt_matrices (k_opt_matrix4_multi across its 36-matrix flush, the other routes in between) and ds2_clip_coef / ds2_opt_multi
through FusedAdamW / FusedSGD (131 tensors: past the 56-tensor table twice, misaligned gradient views) follow."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_reference as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64          # floats before and after every fp32 operand: 256 bytes, the operand keeps its alignment
ROWS = 8            # rows of 7.0 before and after a bf16 window: 8 rows of any stride are a multiple of 16 bytes
ADAMW = dict(lr=1.5e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
SGD = dict(lr=3e-2, momentum=0.9, weight_decay=1e-3)
HP = {0: O.adamw_hp(step=3, **ADAMW), 1: O.sgd_hp(**SGD)}
# name, mode, first, momentum buffer filled with 1e30, v pointer null
VARIANTS = [("adamw", 0, 0, False, False), ("sgd", 1, 0, False, False), ("sgd-first", 1, 1, True, False), ("sgd-no-v", 1, 0, False, True)]
OUTPUTS = [("copy", True, False), ("transpose", False, True), ("neither", False, False), ("both", True, True)]
CS = float(np.float32(0.37))


@pytest.fixture(scope="module")
def lib():
    from deepspeech.pytorch_amd import _lib
    return _lib.load()


def _operands(c, seed):
    """Pristine guarded device buffers of one case and the fp32 operands on the CPU."""
    rs = np.random.RandomState(seed)
    shape = (c["R"], c["C"])
    cpu = dict(p=O.signed(rs, shape), g=O.signed(rs, shape), m=O.signed(rs, shape, 0.1), v=np.abs(O.signed(rs, shape, 0.01)))
    dev = {}
    for k, x in cpu.items():
        off = GUARD + (c["p_offset"] if k == "p" else 0)
        buf = torch.full((off + x.size + GUARD,), 3.0, dtype=torch.float32)
        buf[off:off + x.size] = torch.from_numpy(x.reshape(-1))
        dev[k] = buf.to(DEV)
    return cpu, dev


class Run:
    """Fresh copies of a case's operands and fresh bf16 buffers for one launch."""

    def __init__(self, c, start, v_null=False, want_dst=True, want_dstT=True):
        self.c, self.start, self.v_null = c, start, v_null
        self.n = c["R"] * c["C"]
        self.bufs = {k: t.clone() for k, t in start.items()}
        self.off = {k: GUARD + (c["p_offset"] if k == "p" else 0) for k in "pgmv"}
        self.dst_buf = torch.full((c["R"] + 2 * ROWS, c["ldd"]), 7.0, dtype=torch.bfloat16, device=DEV) if want_dst else None
        self.dstT_buf = torch.full((c["Cout"] + 2 * ROWS, c["lddT"]), 7.0, dtype=torch.bfloat16, device=DEV) if want_dstT else None

    def ptr(self, k):
        if k == "v" and self.v_null:
            return None
        if k in ("dst", "dstT"):
            buf = self.dst_buf if k == "dst" else self.dstT_buf
            return None if buf is None else buf[ROWS:].data_ptr()
        return self.bufs[k][self.off[k]:].data_ptr()

    def shape_args(self):
        c = self.c
        return c["R"], c["C"], c["perm_c"], c["perm_f"], c["Cout"], self.ptr("dst"), c["ldd"], self.ptr("dstT"), c["lddT"]

    def route(self, lib, mode):
        return lib.ds2_opt_matrix_route(mode, self.ptr("p"), self.ptr("g"), self.ptr("m"), self.ptr("v"), *self.shape_args())

    def expected_route(self):
        return self.c["route"] if self.dst_buf is not None else self.c["route_no_dst"]

    def operand(self, k):
        return self.bufs[k][self.off[k]:self.off[k] + self.n].cpu().reshape(self.c["R"], self.c["C"])


WORST = {}


def _check(run, mode, ref, label):
    """Guards, g and an unused v keep their bits; p, m, v are within K of the reference; the layouts are those of the updated p."""
    c = run.c
    assert torch.equal(run.bufs["g"], run.start["g"]), label
    if mode == 1:
        assert torch.equal(run.bufs["v"], run.start["v"]), label                       # SGD: v stays untouched, passed or not
    for k in ("p", "m") + (("v",) if mode == 0 else ()):
        o = run.off[k]
        assert torch.equal(run.bufs[k][:o], run.start[k][:o]) and torch.equal(run.bufs[k][o + run.n:], run.start[k][o + run.n:]), (label, k)
    p = run.operand("p")
    d = O.distances(ref, p, run.operand("m"), run.operand("v") if mode == 0 else None)
    for k, x in d.items():
        key = ("adamw" if mode == 0 else "sgd", k)
        if not x <= WORST.get(key, 0.0):
            WORST[key] = x
            print("largest distance so far: %s %s  K = %.4f of %.4f  (%s)" % (key[0], k, x, O.K, label))
    assert all(x <= O.K for x in d.values()), (label, d, O.K)
    want, wantT = O.layouts(p, c["perm_c"], c["perm_f"], c["Cout"])
    for buf, w in ((run.dst_buf, want), (run.dstT_buf, wantT)):
        if buf is not None:
            full = torch.full(buf.shape, 7.0, dtype=torch.bfloat16)
            full[ROWS:ROWS + w.shape[0], :w.shape[1]] = w
            assert torch.equal(buf.cpu(), full), (label, "transpose" if buf is run.dstT_buf else "copy")


def _same_bits(a, b):
    return all(torch.equal(a.bufs[k], b.bufs[k]) for k in "pgmv") and all(
        (x is None and y is None) or torch.equal(x, y) for x, y in ((a.dst_buf, b.dst_buf), (a.dstT_buf, b.dstT_buf)))


@pytest.mark.parametrize("index", range(len(O.MATRIX_CASES)), ids=[O.case_id(c) for c in O.MATRIX_CASES])
def test_opt_matrix_route_against_the_reference(lib, index):
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd._lib import call
    c = O.MATRIX_CASES[index]
    cpu, dev = _operands(c, 1000 + index)
    for name, mode, first, m_big, v_null in VARIANTS:
        start = dict(dev)
        m0 = cpu["m"]
        if m_big:
            m0 = np.full_like(cpu["m"], 1e30)
            start["m"] = dev["m"].clone()
            start["m"][GUARD:GUARD + m0.size] = 1e30
        hp = (C.c_float * 7)(*HP[mode])
        refs = {cs: O.update(mode, HP[mode], cpu["p"], cpu["g"], m0, cpu["v"], cs=cs, first=first) for cs in (1.0, CS)}
        for out, want_dst, want_dstT in OUTPUTS:
            runs = {}
            for clip in (None, 0.37, 1.0):
                label = "%s %s %s clip %s" % (O.case_id(c), name, out, clip)
                run = runs[clip] = Run(c, start, v_null, want_dst, want_dstT)
                assert run.route(lib, mode) == run.expected_route(), label
                clip_t = None if clip is None else torch.tensor([3.0, clip], dtype=torch.float32, device=DEV)
                call("ds2_opt_matrix", mode, run.ptr("p"), run.ptr("g"), run.ptr("m"), run.ptr("v"), *run.shape_args(), hp, first,
                     ops.P(clip_t), ops.S())
                torch.cuda.synchronize()
                _check(run, mode, refs[CS if clip == 0.37 else 1.0], label)
            assert _same_bits(runs[None], runs[1.0]), label                             # a coefficient of 1 changes no bit
            assert not torch.equal(runs[None].bufs["p"], runs[0.37].bufs["p"]), label   # and 0.37 was read


@pytest.mark.parametrize("index", [1, 17], ids=["matrix4", "generic"])
def test_adamw_eps_is_part_of_the_step(lib, index):
    """Every case above has eps = 1e-8 under a denominator of ~ 1, where a wrong eps moves nothing.  With eps = 0.1 it is a twentieth
    of the denominator (the reference with 1e-8 is far outside K), and the kernels' one shared update must still meet the bounds."""
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd._lib import call
    c = O.MATRIX_CASES[index]
    cpu, dev = _operands(c, 3000 + index)
    hp = O.adamw_hp(step=3, **dict(ADAMW, eps=O.BIG_EPS))
    ref = O.update(0, hp, cpu["p"], cpu["g"], cpu["m"], cpu["v"], cs=CS)
    small = O.update(0, HP[0], cpu["p"], cpu["g"], cpu["m"], cpu["v"], cs=CS)
    assert O.distance(small["p"].astype(np.float32), ref["p"], ref["p_scale"]) > 1e3
    run = Run(c, dev)
    assert run.route(lib, 0) == c["route"]
    clip_t = torch.tensor([3.0, 0.37], dtype=torch.float32, device=DEV)
    call("ds2_opt_matrix", 0, run.ptr("p"), run.ptr("g"), run.ptr("m"), run.ptr("v"), *run.shape_args(), (C.c_float * 7)(*hp), 0,
         ops.P(clip_t), ops.S())
    torch.cuda.synchronize()
    _check(run, 0, ref, "%s adamw eps %g" % (O.case_id(c), O.BIG_EPS))


@pytest.mark.parametrize("mode", [0, 1])
def test_opt_matrices_against_the_reference(lib, mode):
    """One ds2_opt_matrices call: 38 matrices of route 0 -- k_opt_matrix4_multi, flushed after the 36th -- with one matrix of each
    other route in between, some without a copy, some without a transpose, clipped by 0.37.  Every matrix against the reference."""
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd._lib import call
    rs = np.random.RandomState(90 + mode)
    cases = [O._case(O.MATRIX4, 16 * int(rs.randint(1, 5)), 4 * int(rs.randint(1, 41))) for _ in range(38)]
    cases.insert(10, O._case(O.PERM_ROWS, 32, 40, 48, (8, 5)))
    cases.insert(20, O._case(O.PERM, 16, 20, 24, (4, 5)))
    cases.insert(30, O._case(O.GENERIC, 48, 202))
    runs, refs = [], []
    for k, c in enumerate(cases):
        cpu, dev = _operands(c, 2000 + 100 * mode + k)
        runs.append(Run(c, dev, False, k % 5 != 3, k % 7 != 2))
        refs.append(O.update(mode, HP[mode], cpu["p"], cpu["g"], cpu["m"], cpu["v"], cs=CS))
        assert runs[-1].route(lib, mode) == runs[-1].expected_route() == c["route"], k
    assert [r.c["route"] for r in runs].count(O.MATRIX4) == 38 and {r.c["route"] for r in runs} == {0, 1, 2, 3}
    assert any(r.dst_buf is None for r in runs) and any(r.dstT_buf is None for r in runs)
    parr = lambda k: (C.c_void_p * len(runs))(*[r.ptr(k) for r in runs])
    iarr = lambda k: (C.c_int * len(runs))(*[r.c[k] for r in runs])
    larr = lambda k: (C.c_long * len(runs))(*[r.c[k] for r in runs])
    clip_t = torch.tensor([3.0, 0.37], dtype=torch.float32, device=DEV)
    call("ds2_opt_matrices", mode, len(runs), parr("p"), parr("g"), parr("m"), parr("v"), iarr("R"), iarr("C"), iarr("perm_c"), iarr("perm_f"),
         iarr("Cout"), parr("dst"), larr("ldd"), parr("dstT"), larr("lddT"), (C.c_float * 7)(*HP[mode]), 0, ops.P(clip_t), ops.S())
    torch.cuda.synchronize()
    for k, (run, ref) in enumerate(zip(runs, refs)):
        _check(run, mode, ref, "ds2_opt_matrices mode %d matrix %d %s" % (mode, k, O.case_id(run.c)))


# ---- ds2_clip_coef + ds2_opt_multi through the optimizers ---------------------------------------------------------------------
BIG, NONE_GRAD, STRIDED = 60, 3, 7
GROUP0 = 120                                    # parameters of the first group: its ds2_opt_multi crosses the 56-tensor table twice
GROUP1 = dict(adamw=dict(lr=4e-3, weight_decay=5e-2), sgd=dict(lr=1e-2, weight_decay=5e-3))


def _shapes():
    rs = np.random.RandomState(7)
    shapes = [(int(rs.randint(1, 41)),) for _ in range(130)]
    shapes[STRIDED] = (5, 7)
    shapes.insert(BIG, (16385,))
    return shapes


class Trainer:
    """131 parameters in two groups under FusedAdamW / FusedSGD.  Gradients: views into ONE flat buffer from element 1 on (most
    of them off 16-byte alignment, the 16 385-element one included: the scalar branch of k_sumsq over two workgroups), one that is a
    transposed view (copied by the optimizer), one parameter without a gradient."""

    def __init__(self, mode, clip):
        from deepspeech.pytorch_amd.optim import FusedAdamW, FusedSGD
        self.mode, self.shapes = mode, _shapes()
        rs = np.random.RandomState(11)
        self.params = [torch.nn.Parameter(torch.from_numpy(O.signed(rs, s)).to(DEV)) for s in self.shapes]
        groups = [dict(params=self.params[:GROUP0]), dict(params=self.params[GROUP0:], **GROUP1["adamw" if mode == 0 else "sgd"])]
        self.opt = FusedAdamW(groups, clip_grad_norm=clip, **ADAMW) if mode == 0 else FusedSGD(groups, clip_grad_norm=clip, **SGD)
        sizes = [int(np.prod(s)) for s in self.shapes]
        lead = 1 if (1 + sum(sizes[:BIG])) % 4 else 2          # the large gradient, too, starts off 16-byte alignment
        self.flat = torch.zeros(lead + sum(sizes), dtype=torch.float32, device=DEV)
        self.strided = torch.zeros((7, 5), dtype=torch.float32, device=DEV)
        at = lead
        for i, (p, s, n) in enumerate(zip(self.params, self.shapes, sizes)):
            if i == STRIDED:
                p.grad = self.strided.t()
            elif i != NONE_GRAD:
                p.grad = self.flat[at:at + n].view(s)
            at += n
        assert not self.params[STRIDED].grad.is_contiguous() and self.params[BIG].grad.data_ptr() % 16 != 0
        assert sum(p.grad is not None and p.grad.data_ptr() % 16 != 0 for p in self.params) > 64

    def set_grads(self, seed, zero=False):
        rs = np.random.RandomState(seed)
        scale = 0.0 if zero else 1.0
        self.flat.copy_(torch.from_numpy(O.signed(rs, self.flat.shape, scale)))
        self.strided.copy_(torch.from_numpy(O.signed(rs, (7, 5), scale)))

    def moments(self, p):
        st = self.opt.state[p]
        if self.mode == 0:
            return (st["exp_avg"].clone(), st["exp_avg_sq"].clone()) if st else (torch.zeros_like(p), torch.zeros_like(p))
        return (st["momentum_buffer"].clone() if st else torch.zeros_like(p)), None

    def snapshot(self):
        return [(p.detach().clone(),) + self.moments(p) for p in self.params]

    def hp(self, group, step):
        g = self.opt.param_groups[group]
        if self.mode == 0:
            return O.adamw_hp(g["lr"], g["betas"], g["eps"], g["weight_decay"], step)
        return O.sgd_hp(g["lr"], g["momentum"], g["weight_decay"])

    def clip_out(self):
        norm, coef = self.opt._clip_out[self.params[0].device].cpu().tolist()
        assert norm == float(self.opt.last_grad_norm[self.params[0].device])
        return norm, coef


def _check_step(t, before, step, cs, label):
    after = t.snapshot()
    for i, (p, b, a) in enumerate(zip(t.params, before, after)):
        if p.grad is None:
            assert torch.equal(a[0], b[0]) and len(t.opt.state[p]) == 0, (label, i)
            continue
        ref = O.update(t.mode, t.hp(0 if i < GROUP0 else 1, step), b[0], p.grad, b[1], b[2], cs=cs, first=int(step == 1))
        d = O.distances(ref, a[0], a[1], a[2])
        for k, x in d.items():
            key = ("multi adamw" if t.mode == 0 else "multi sgd", k)
            if not x <= WORST.get(key, 0.0):
                WORST[key] = x
                print("largest distance so far: %s %s  K = %.4f of %.4f  (%s, parameter %d)" % (key[0], k, x, O.K, label, i))
        assert all(x <= O.K for x in d.values()), (label, i, d, O.K)


@pytest.mark.parametrize("mode", [0, 1])
def test_clip_and_multi_tensor_update_past_the_table_size(lib, mode):
    """Three steps, clipped (coefficient ~ 0.35): the norm and the coefficient against the float64 clip reference, every parameter
    and moment of every step against the float64 update from the state before the step, with the device's own coefficient as cs."""
    assert lib.ds2_opt_max_tensors() == 56
    t = Trainer(mode, 50.0)
    assert len(t.params) == 131 and len(t.opt.param_groups[0]["params"]) > 2 * 56
    for step in (1, 2, 3):
        t.set_grads(100 * mode + step)
        before = t.snapshot()
        t.opt.step()
        norm, coef = t.clip_out()
        norm_ref, coef_ref = O.clip_reference([p.grad for p in t.params if p.grad is not None], 50.0)
        print("step %d: norm %.9g (float64 %.9g), coefficient %.9g (float64 %.9g)" % (step, norm, norm_ref, coef, coef_ref))
        assert coef_ref < 0.5
        assert abs(norm - norm_ref) <= O.CLIP_RTOL * norm_ref and abs(coef - coef_ref) <= O.CLIP_RTOL * coef_ref
        _check_step(t, before, step, coef, "mode %d step %d" % (mode, step))


@pytest.mark.parametrize("mode", [0, 1])
def test_a_clip_far_above_the_norm_changes_no_bit(mode):
    runs = {}
    for clip in (None, 1e6):
        t = runs[clip] = Trainer(mode, clip)
        for step in (1, 2, 3):
            t.set_grads(300 + step)
            before = t.snapshot()
            t.opt.step()
            if clip is not None:
                assert t.clip_out()[1] == 1.0
        _check_step(t, before, 3, 1.0, "mode %d clip %s step 3" % (mode, clip))
    for (a, b) in zip(runs[None].snapshot(), runs[1e6].snapshot()):
        assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("mode", [0, 1])
def test_an_all_zero_gradient_gives_coefficient_one(mode):
    """Norm 0: max_norm / (0 + 1e-6) is clamped to 1, and the step is the un-clipped one (AdamW: only the weight decay moves p)."""
    t = Trainer(mode, 0.75)
    t.set_grads(0, zero=True)
    before = t.snapshot()
    t.opt.step()
    assert t.clip_out() == (0.0, 1.0)
    if mode == 0:               # SGD's buffer is wd * p0 here, which the m measure (|m0| + |cs g| = 0) has no room for
        _check_step(t, before, 1, 1.0, "mode %d zero gradient" % mode)
    else:
        hp = t.hp(0, 1)
        for p, b in zip(t.params[:GROUP0], before):
            if p.grad is not None:
                want = O.f64(b[0]) * (1.0 + hp[6] * hp[0] * (1.0 + hp[1]))          # p0 - lr (wd p0 + momentum wd p0)
                assert (np.abs(O.f64(p) - want) <= O.K * O.ULP * np.abs(want)).all()
