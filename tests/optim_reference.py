"""Float64 reference of the optimizer step of csrc/ds2_optim.hip, plain numpy / torch on the CPU, no device and no kernel of
this project: one step of AdamW or SGD-Nesterov from fp32 inputs, the global-norm clip coefficient, and the bf16 copy / transpose
a matrix kernel leaves next to the updated matrix.  tests/test_optim_reference_host.py holds it against torch.optim on the CPU,
tests/test_gpu_optim_routes.py holds every kernel route against it.

The update.  update() takes the fp32 operands p0, g, m0, v0 as they are (exactly representable in float64), the hyper-parameter
vector as optim.py builds it (adamw_hp / sgd_hp: python doubles, NOT rounded to float -- the kernels receive it as floats, and that
rounding is part of their distance from this reference, as it is part of torch's), a clip coefficient cs and SGD's `first`:

  AdamW   gc = cs g;  m = m0 + w1 (gc - m0);  v = beta2 v0 + w2 gc^2;  p = decay p0 + neg_step m / (sqrt(v) / bc2_sqrt + eps)
  SGD     gd = cs g + wd p0;  m = gd on the first step, else momentum m0 + gd;  p = p0 + neg_step (gd + momentum m)

The tolerance of the fp32 results, per element, with ulp = 2^-23 and `step` = p_ref - p0:

  |v - v_ref| <= K ulp |v_ref|        |m - m_ref| <= K ulp (|m0| + |cs g|)        |p - p_ref| <= K ulp (|p0| + |step|)

(SGD's first step ignores m0, so its |m0| term is 0 there: the test fills m0 with 1e30, which would make the bound empty.)
distance() returns the smallest K an array meets, so a test can print it before it asserts.

The operands.  The measures divide by |p0| + |step| and |m0| + |cs g|.  An element where these are small next to a term they
leave out -- wd p0 in SGD's buffer when g is nearly zero, a step that cancels against a parameter that is nearly zero -- needs
an arbitrarily large K for a correctly rounded fp32 result: with standard normal operands torch's own fp32 SGD shows K = 35 823
on m and 16.3 on p, its AdamW 6.4 on p, each from the single unluckiest of 83 000 elements.  A K set by such an element holds
all the others to nothing, and twice the largest of one draw does not bound the next draw.  So every test here draws p, g (and
the starting moments, m0 at a tenth and v0 >= 0 at a hundredth of that) as signed(): magnitude U(0.5, 1.5), random sign.  No
denominator is small then, the measures are well-conditioned, and the largest distance is a property of the arithmetic, not of
the draw.  The bounds still see a relative error of 1e-5 in the step (lr ~ 1e-2 against |p0| ~ 1) and of 1e-6 in m and v.

K is not taken from the kernels.  test_optim_reference_host.py runs torch.optim.AdamW / SGD(nesterov) (foreach=False) with
clip_grad_norm_ on the CPU in fp32 for three steps over the shapes of tests/test_gpu_optim.py, and one step from injected
non-zero moments (the state the GPU cases start from), unclipped, clipped hard (coefficient ~ 0.003) and clipped mildly (~ 0.35),
and AdamW again with eps = BIG_EPS (eps as large as the rest of the denominator, the one setting in which a wrong eps shows), each
step against update() from torch's own fp32 state before the step.  The largest distance torch shows there:

  AdamW  v 2.2333 (first step, clipped hard)   p 1.1913   m 0.4851          SGD  m 1.8477   p 0.6011

  K_TORCH = 2.2333,  K = 2 K_TORCH = 4.4666

The kernels follow torch statement by statement; the factor 2 is for FMA contraction on the device, which rounds each of the
two or three dependent operations of a statement differently.

The clip.  clip_reference(): norm = float64 sqrt of the float64 sum of squares, coef = min(1, max_norm / (norm + 1e-6)).  Norm and
coefficient are held to the project's 1e-5 relative bar (CLIP_RTOL).  The per-element bounds above take cs as an INPUT: a test feeds
update() the fp32 coefficient the device (or torch) computed, after holding that coefficient to clip_reference(); a coefficient off
by 1e-5 is 84 ulp of every gradient and must not be charged to the update.

The layouts.  layouts() starts from the updated fp32 matrix the kernel itself left in p: bf16 copy [R][Cout] = p.to(bfloat16),
columns re-ordered f * perm_c + c <- c * perm_f + f under a permutation, columns [C, Cout) zero; the transpose is .t() of that.
They are compared bit for bit (torch.equal), whatever the update's tolerance."""
import numpy as np
import torch

ULP = 2.0 ** -23
K_TORCH = 2.2333
K = 2 * K_TORCH
CLIP_RTOL = 1e-5
BIG_EPS = 0.1          # an AdamW eps of the denominator's own size (sqrt(v) / bc2_sqrt ~ 1 here): at 1e-8 no bound notices a wrong eps

TENSOR_SHAPES = [(7,), (33, 5), (16384,), (16385,), (3, 41, 11), (50000,), (96, 40), (1,)]     # those of tests/test_gpu_optim.py


def signed(rs, shape, scale=1.0):
    """fp32 operands of magnitude scale * U(0.5, 1.5) and random sign (see `The operands` above)."""
    return (scale * rs.uniform(0.5, 1.5, shape) * rs.choice([-1.0, 1.0], shape)).astype(np.float32)


def tensors(seed):
    rs = np.random.RandomState(seed)
    return [signed(rs, s) for s in TENSOR_SHAPES]


def adamw_hp(lr, betas, eps, weight_decay, step):
    """hp of FusedAdamW.step (optim.py), python doubles."""
    beta1, beta2 = betas
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    return [1 - lr * weight_decay, 1 - beta1, beta2, 1 - beta2, bc2 ** 0.5, eps, -(lr / bc1)]


def sgd_hp(lr, momentum, weight_decay):
    """hp of FusedSGD.step (optim.py)."""
    return [weight_decay, momentum, 0.0, 0.0, 1.0, 0.0, -lr]


def f64(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def update(mode, hp, p0, g, m0, v0=None, cs=1.0, first=0):
    """One step in float64.  Returns p, m, v (None for SGD) and the scales of the three bounds."""
    p0, g, m0 = f64(p0), f64(g), f64(m0)
    decay, w1, beta2, w2, bc2_sqrt, eps, neg_step = [float(x) for x in hp]
    gc = float(cs) * g
    if mode == 0:
        v0 = f64(v0)
        m = m0 + w1 * (gc - m0)
        v = v0 * beta2 + w2 * gc * gc
        p = p0 * decay + neg_step * m / (np.sqrt(v) / bc2_sqrt + eps)
        m_old = np.abs(m0)
    else:
        gd = gc + decay * p0
        m = gd if first else m0 * w1 + gd
        v = None
        p = p0 + neg_step * (gd + w1 * m)
        m_old = 0.0 if first else np.abs(m0)
    return dict(p=p, m=m, v=v, p_scale=np.abs(p0) + np.abs(p - p0), m_scale=m_old + np.abs(gc), v_scale=None if v is None else np.abs(v))


def distance(got, ref, scale):
    """max over the elements of |got - ref| / (ulp * scale): the K this array needs.  A scale of zero admits only the exact value."""
    err = np.abs(f64(got) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / (ULP * scale))
    return float(r.max())


def distances(ref, p, m, v=None):
    """{'p': K, 'm': K, 'v': K} of fp32 results against update()'s output."""
    d = dict(p=distance(p, ref["p"], ref["p_scale"]), m=distance(m, ref["m"], ref["m_scale"]))
    if ref["v"] is not None:
        d["v"] = distance(v, ref["v"], ref["v_scale"])
    return d


def clip_reference(grads, max_norm):
    """(norm, coefficient) of torch.nn.utils.clip_grad_norm_ in float64."""
    norm = float(np.sqrt(sum(float((f64(g) ** 2).sum()) for g in grads)))
    return norm, min(1.0, float(max_norm) / (norm + 1e-6))


def layouts(p, perm_c, perm_f, Cout):
    """(bf16 copy [R][Cout], bf16 transpose [Cout][R]) of the fp32 matrix p on the CPU."""
    p = p.detach().cpu()
    R, C = p.shape
    b = p.to(torch.bfloat16)
    if perm_c > 0:
        b = b.reshape(R, perm_c, perm_f).permute(0, 2, 1).reshape(R, C)
    out = torch.zeros((R, Cout), dtype=torch.bfloat16)
    out[:, :C] = b
    return out, out.t().contiguous()


# ---- the matrix cases of tests/test_gpu_optim_routes.py, shared with the routing table of tests/test_optim_reference_host.py
MATRIX4, PERM_ROWS, PERM, GENERIC = 0, 1, 2, 3


def _case(route, R, C, Cout=None, perm=(0, 0), ldd=None, p_offset=0, route_no_dst=None):
    Cout = C if Cout is None else Cout
    ldd = Cout + 8 if ldd is None else ldd
    return dict(route=route, route_no_dst=route if route_no_dst is None else route_no_dst, R=R, C=C, Cout=Cout, perm_c=perm[0],
                perm_f=perm[1], ldd=ldd, lddT=R + 8, p_offset=p_offset)


# (R; C or perm_c x perm_f; Cout).  ldd = Cout + 8 unless given (always > Cout), lddT = R + 8.  route_no_dst: the route when no
# bf16 copy is asked for, where the copy's row stride is what keeps the case off a faster kernel.
MATRIX_CASES = [
    _case(MATRIX4, 16, 4), _case(MATRIX4, 16, 64, ldd=68), _case(MATRIX4, 80, 68), _case(MATRIX4, 48, 200),
    _case(PERM_ROWS, 16, 1312, 1344, (32, 41)), _case(PERM_ROWS, 96, 1312, 1344, (32, 41)),            # cw = 16, two channel blocks
    _case(PERM_ROWS, 32, 40, 40, (8, 5)), _case(PERM_ROWS, 32, 40, 48, (8, 5)),                        # cw = perm_c, one block
    _case(PERM_ROWS, 16, 48, 48, (16, 3)), _case(PERM_ROWS, 32, 16, 24, (8, 2)),                       # channel wraps inside a quad
    _case(PERM_ROWS, 16, 4096, 4096, (32, 128)),                                                       # exactly PR_MAX_LDS
    _case(PERM, 16, 20, 20, (4, 5)), _case(PERM, 16, 20, 24, (4, 5)),
    _case(PERM, 80, 84, 96, (12, 7)),                                                                  # two column tiles, ragged rows
    _case(PERM, 16, 4128, 4128, (32, 129)),                                                            # one past the LDS limit
    _case(PERM, 96, 1312, 1344, (32, 41), ldd=1348, route_no_dst=PERM_ROWS),
    _case(GENERIC, 16, 1, ldd=3), _case(GENERIC, 16, 63, ldd=71), _case(GENERIC, 80, 65), _case(GENERIC, 48, 202),
    _case(GENERIC, 32, 40, 64), _case(GENERIC, 32, 40, 136),                                           # a column tile of padding only
    _case(GENERIC, 16, 21, 21, (3, 7)), _case(GENERIC, 16, 21, 24, (3, 7)), _case(GENERIC, 80, 65, 72, (5, 13)),
    _case(GENERIC, 64, 64, p_offset=1),                                                                # p off by one float
]


def case_id(c):
    shape = "%dx%d" % (c["perm_c"], c["perm_f"]) if c["perm_c"] else "%d" % c["C"]
    return "%s-%d-%s-%d-ldd%d%s" % (("matrix4", "perm_rows", "perm", "generic")[c["route"]], c["R"], shape, c["Cout"], c["ldd"],
                                    "-p+1" if c["p_offset"] else "")
