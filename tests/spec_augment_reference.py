"""Restatement in numpy fp64 of what the reference's ``spec_augment`` (loader/spec_augment.py:48-115) computes on one F x T
spectrogram, written from the rules and not from its code path (loader/sparse_image_warp.py:88-411 builds a dense flow field and
gathers four corners; with ONE control point that collapses to the closed forms below).

Time warp: control point source (F//2, pt), destination c = (F//2, pt + d) with pt = spec[F//2][i] (a spectrogram VALUE used as a
time coordinate, spec_augment.py:56-62).  The order-2 polyharmonic system is [[0, c^T], [c, E]] (c extended by 1, E the 3 x 3
block of randn / 1e10, sparse_image_warp.py:170), right-hand side (0, d) for the (frequency, time) flow components:
    w = -d / (c^T E^-1 c),   v = d * E^-1 c / (c^T E^-1 c)            (E^-1 = adj(E) / det(E): the determinant cancels in v)
The frequency component is exactly zero.  The radial term phi(r) * w is evaluated at r = S - 2 q.c + |c|^2 where S sums the squared
norms of ALL grid points into one scalar (cross_squared_distance_matrix, :197-198), so it is the constant K = w * phi(S + |c|^2) up
to a position dependence of relative size |q.c| / S that w ~ 1e-10 scales to nothing.  flow_t(f, t) = a_f f + a_t t + a_0 with
(a_f, a_t, a_0) = (v_0, v_1, v_2 + K).

Warp: out[f][t] = x[f][fl] + alpha * (x[f][fl + 1] - x[f][fl]),  q = t - flow_t(f, t),  fl = clamp(floor(q), 0, T - 2),
alpha = clamp(q - fl, 0, 1)  (interpolate_bilinear, :357-408).  All-zero coefficients mean "no warp": the clip is copied.
Masks: rows [f0, f0 + f) and frames [t0, t0 + w) are zeroed (spec_augment.py:98-113)."""
import numpy as np


def grid_norm(F, T):
    """sum over the F x T grid of f^2 + t^2."""
    return T * ((F - 1) * F * (2 * F - 1) // 6) + F * ((T - 1) * T * (2 * T - 1) // 6)


def phi2(r):
    return 0.5 * r * np.log(max(r, 1e-10))


def warp_coef(F, T, pt, i, d, E, W=5):
    """(a_f, a_t, a_0) in fp64 from the draw; zeros when the warp is off (i < 0) or the clip has T <= 2W frames (the reference's
    randrange raises there)."""
    if i < 0 or T <= 2 * W:
        return np.zeros(3)
    c = np.array([F // 2, float(np.float32(np.float32(pt) + np.float32(d))), 1.0])     # the reference holds c in fp32
    E = np.asarray(E, np.float64).reshape(3, 3)
    adj = np.array([[E[1, 1] * E[2, 2] - E[1, 2] * E[2, 1], E[0, 2] * E[2, 1] - E[0, 1] * E[2, 2], E[0, 1] * E[1, 2] - E[0, 2] * E[1, 1]],
                    [E[1, 2] * E[2, 0] - E[1, 0] * E[2, 2], E[0, 0] * E[2, 2] - E[0, 2] * E[2, 0], E[0, 2] * E[1, 0] - E[0, 0] * E[1, 2]],
                    [E[1, 0] * E[2, 1] - E[1, 1] * E[2, 0], E[0, 1] * E[2, 0] - E[0, 0] * E[2, 1], E[0, 0] * E[1, 1] - E[0, 1] * E[1, 0]]])
    det = E[0] @ adj[:, 0]
    u = adj @ c
    q = c @ u                                   # c^T adj(E) c = det * c^T E^-1 c
    coef = d * u / q
    coef[2] += (-d * det / q) * phi2(grid_norm(F, T) + c[0] * c[0] + c[1] * c[1])
    return coef


def warp(x, coef):
    x = np.asarray(x, np.float64)
    F, T = x.shape
    coef = np.asarray(coef, np.float64)
    if not coef.any():
        return x.copy()
    f = np.arange(F, dtype=np.float64)[:, None]
    t = np.arange(T, dtype=np.float64)[None, :]
    q = t - (coef[0] * f + coef[1] * t + coef[2])
    fl = np.clip(np.floor(q), 0, T - 2)
    al = np.clip(q - fl, 0.0, 1.0)
    fl = fl.astype(np.int64)
    rows = np.arange(F)[:, None]
    lo, hi = x[rows, fl], x[rows, fl + 1]
    return lo + al * (hi - lo)


def apply_masks(y, fmask, tmask):
    y = y.copy()
    for f0, w in np.asarray(fmask, np.int64).reshape(-1, 2):
        y[f0:f0 + w, :] = 0
    for t0, w in np.asarray(tmask, np.int64).reshape(-1, 2):
        y[:, t0:t0 + w] = 0
    return y


def spec_augment(x, coef, fmask, tmask):
    return apply_masks(warp(x, coef), fmask, tmask)


def in_mask(F, T, fmask, tmask):
    """boolean F x T: cells that a mask zeroes."""
    m = np.zeros((F, T), bool)
    for f0, w in np.asarray(fmask, np.int64).reshape(-1, 2):
        m[f0:f0 + w, :] = True
    for t0, w in np.asarray(tmask, np.int64).reshape(-1, 2):
        m[:, t0:t0 + w] = True
    return m
