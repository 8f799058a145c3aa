#!/usr/bin/env python3
"""Generate the SpecAugment fixtures tests/golden/specaug/*.npz from the REAL reference: ``loader/sparse_image_warp.py`` imported
unmodified, ``loader/spec_augment.py`` imported unmodified with stub ``librosa`` / ``matplotlib`` modules (it imports them for its
plotting helper only).  Run in the build container only:

    python tests/golden/make_spec_augment.py      # rewrites tests/golden/specaug/*.npz and prints one line per fixture

Two kinds of fixture:
  e2e_*   ``spec_augment(spect)`` itself under seeded ``random`` / ``numpy.random`` / ``torch`` generators; the draws are replayed
          from the same seeds and recorded (frame index i, shift d, the 3 x 3 block E, mask widths and starts).
  hand_*  chosen (i, d, E seed) through ``sparse_image_warp`` directly, then chosen masks applied as spec_augment.py:104/113 do
          (assignment of 0): masks at the edges, of width 0, across bins 64 and 128, flows that clamp at either end.
Every file holds: x (F, T) f32 input, i, d, pt = x[F//2][i], E (9) f32, fmask (MF, 2) / tmask (MT, 2) int32 [start, width],
w (2) / v (3, 2) of solve_interpolation, coef_ref (3) f64 = least-squares affine fit (a_f, a_t, a_0) of the dense time flow with
fit_resid = its largest residual, flow_f_absmax = largest |frequency flow| (0), flow_absmax, out (F, T) f32 reference output.
Seeds are searched for the CONDITION ON THE INPUTS max |flow| <= 2T (a draw with c^T E^-1 c near 0 gives an unbounded flow whose
output is a constant row per bin and proves nothing); the generator asserts it.  Nothing here is used by the product path."""
import importlib
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from ref_harness import REFERENCE_ROOT  # noqa: E402
import spec_augment_reference as R  # noqa: E402

OUT = os.path.join(HERE, "specaug")
W = 5


def load_reference():
    for name in ("librosa", "librosa.display", "matplotlib", "matplotlib.pyplot"):
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except Exception:
                m = types.ModuleType(name)
                m.use = lambda *a, **k: None              # matplotlib.use('Agg'), spec_augment.py:42
                sys.modules[name] = m
    pkg = types.ModuleType("ref_loader")
    pkg.__path__ = [os.path.join(REFERENCE_ROOT, "deepspeech_pytorch", "loader")]
    sys.modules["ref_loader"] = pkg
    siw = importlib.import_module("ref_loader.sparse_image_warp")
    sa = importlib.import_module("ref_loader.spec_augment")
    return siw, sa


def make_spect(F, T, seed):
    """normalised (mean 0, std 1) fp32 field with energy at every frame-to-frame scale, like data_loader.py:88-92 leaves it."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((F, T)) + 2.0 * np.sin(np.arange(T)[None, :] * 0.31 + np.arange(F)[:, None] * 0.07)
    x = (x - x.mean()) / x.std(ddof=1)
    return x.astype(np.float32)


def affine_fit(flow_t):
    F, T = flow_t.shape
    f, t = np.meshgrid(np.arange(F, dtype=np.float64), np.arange(T, dtype=np.float64), indexing="ij")
    A = np.stack([f.ravel(), t.ravel(), np.ones(F * T)], 1)
    y = flow_t.astype(np.float64).ravel()
    coef = np.linalg.lstsq(A, y, rcond=None)[0]
    return coef, float(np.abs(A @ coef - y).max())


class Recorder:
    """wraps the reference's own functions (by attribute, the source stays unmodified) to keep what they return."""

    def __init__(self, siw, sa):
        self.siw, self.sa = siw, sa
        self.solve, self.warp = siw.solve_interpolation, siw.sparse_image_warp
        siw.solve_interpolation = self._solve
        sa.sparse_image_warp = self._warp

    def _solve(self, *a, **k):
        self.w, self.v = self.solve(*a, **k)
        return self.w, self.v

    def _warp(self, img, src, dst, *a, **k):
        self.src, self.dst = src, dst
        out, self.flows = self.siw.sparse_image_warp(img, src, dst, *a, **k)
        return out, self.flows


def record(name, x, i, d, E, fmask, tmask, rec, out):
    F, T = x.shape
    flows = rec.flows[0].numpy()
    coef, resid = affine_fit(flows[..., 1])
    flow_absmax = float(np.abs(flows[..., 1]).max())
    assert flow_absmax <= 2 * T, (name, flow_absmax)                       # the condition on the inputs
    assert float(rec.src[0, 0, 1]) == float(x[F // 2, i]) and float(rec.src[0, 0, 0]) == F // 2
    assert float(rec.dst[0, 0, 1]) == float(np.float32(x[F // 2, i] + np.float32(d)))
    # the replayed E is the block the solve used: rows 1..3 of lhs @ X = 0 hold with it to fp32 rounding
    c = np.array([F // 2, float(rec.dst[0, 0, 1]), 1.0])
    w, v = rec.w[0, 0].numpy().astype(np.float64), rec.v[0].numpy().astype(np.float64)
    lower = c * w[1] + E.astype(np.float64).reshape(3, 3) @ v[:, 1]
    assert np.abs(lower).max() <= 1e-4 * np.abs(c * w[1]).max(), (name, lower)
    assert abs(c @ v[:, 1] - d) <= 1e-3 * max(1, abs(d)), (name, c @ v[:, 1], d)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), x=x, i=np.int32(i), d=np.int32(d), pt=x[F // 2, i], E=E.reshape(9),
                        fmask=np.asarray(fmask, np.int32).reshape(-1, 2), tmask=np.asarray(tmask, np.int32).reshape(-1, 2),
                        w=rec.w[0, 0].numpy(), v=rec.v[0].numpy(), coef_ref=coef, fit_resid=resid,
                        flow_f_absmax=float(np.abs(flows[..., 0]).max()), flow_absmax=flow_absmax, out=out.astype(np.float32))
    q = np.arange(T)[None, :] - flows[..., 1]
    print("%-22s F %3d T %3d i %3d d %2d coef (%.3e %.3e %.3e) resid %.1e |flow| %.2f  q in [%.1f, %.1f]  fmask %s tmask %s"
          % (name, F, T, i, d, coef[0], coef[1], coef[2], resid, flow_absmax, q.min(), q.max(),
             np.asarray(fmask).tolist(), np.asarray(tmask).tolist()))


def replay_E(seed):
    torch.manual_seed(seed)
    return (torch.randn((1, 3, 3)) / 1e10)[0].numpy()


def e2e(rec, F, T, data_seed):
    """the first seed from data_seed * 1000 on whose flow meets the condition."""
    x = make_spect(F, T, data_seed)
    for seed in range(data_seed * 1000, data_seed * 1000 + 200):
        random.seed(seed), np.random.seed(seed), torch.manual_seed(seed)
        out = rec.sa.spec_augment(torch.from_numpy(x.copy())).numpy()
        if float(rec.flows[0, ..., 1].abs().max()) > 2 * T:
            continue
        random.seed(seed), np.random.seed(seed)
        i, d = random.randrange(W, T - W), random.randrange(-W, W)                        # spec_augment.py:56,60
        fw = int(np.random.uniform(low=0.0, high=27))                                     # :99-103
        fmask = [[random.randint(0, F - fw), fw]] if F - fw >= 0 else [[0, 0]]          # :101 skips a mask wider than the axis
        tw =int(np.random.uniform(low=0.0, high=70))                                     # :108-112
        tmask = [[random.randint(0, T - tw), tw]] if T - tw >= 0 else [[0, 0]]
        record("e2e_f%d_t%d" % (F, T), x, i, d, replay_E(seed), fmask, tmask, rec, out)
        return
    raise AssertionError("no seed with a bounded flow for F %d T %d" % (F, T))


def hand(rec, name, F, T, data_seed, fmask, tmask, want):
    """searches (seed, i, d) for a flow whose query frames t - flow satisfy `want(qmin, qmax)`; masks as given."""
    x = make_spect(F, T, data_seed)
    for seed in range(data_seed * 1000, data_seed * 1000 + 400):
        rs = random.Random(seed)
        i, d = rs.randrange(W, T - W), rs.randrange(-W, W)
        if d == 0:
            continue
        pt = torch.from_numpy(x)[F // 2][i]
        torch.manual_seed(seed)
        out, flows = rec.sa.sparse_image_warp(torch.from_numpy(x.copy())[None], torch.tensor([[[F // 2, pt]]]),
                                              torch.tensor([[[F // 2, pt + d]]]))
        ft = flows[0, ..., 1].numpy()
        q = np.arange(T)[None, :] - ft
        if np.abs(ft).max() > 2 * T or not want(q.min(), q.max(), T):
            continue
        out = out[0, ..., 0].numpy().copy()
        for f0, fw in fmask:
            out[f0:f0 + fw, :] = 0
        for t0, tw in tmask:
            out[:, t0:t0 + tw] = 0
        record(name, x, i, d, replay_E(seed), fmask, tmask, rec, out)
        return
    raise AssertionError("no draw found for " + name)


def main():
    os.makedirs(OUT, exist_ok=True)
    siw, sa = load_reference()
    rec = Recorder(siw, sa)
    for n, (F, T) in enumerate([(161, 12), (161, 63), (161, 64), (161, 65), (161, 130), (81, 40), (5, 12)]):
        e2e(rec, F, T, 31 + n)
    inside = lambda lo, hi, T: lo >= 0 and hi <= T - 1                      # noqa: E731
    # masks at f0 = 0, ending at F, of width 0 and across bins 64 and 128 (the 64-bin tiles of the write kernel); time mask to T
    hand(rec, "hand_masks_edges", 161, 65, 41, [[0, 5], [60, 10], [120, 20], [150, 11]], [[0, 3], [30, 0], [58, 7]], inside)
    hand(rec, "hand_masks_width0", 161, 64, 42, [[161, 0], [0, 0]], [[64, 0]], inside)
    hand(rec, "hand_clamp_left", 161, 65, 43, [[70, 0]], [[10, 4]], lambda lo, hi, T: lo < -2 and hi <= T - 1)
    hand(rec, "hand_clamp_right", 161, 65, 44, [[64, 1]], [[64, 1]], lambda lo, hi, T: hi > T + 1 and lo >= 0)
    hand(rec, "hand_clamp_both_f81", 81, 130, 45, [[80, 1]], [[0, 70]], lambda lo, hi, T: hi > T + 1 and lo < -2)
    write_noise_figures()


def write_noise_figures():
    """max |fp64 restatement - reference output| per fixture: the fp32 noise of the reference itself, the yardstick of the device
    tests.  Kept as reference_noise.json (read by the tests) and as a table in README.md."""
    import glob
    import json
    fig = {}
    for p in sorted(glob.glob(os.path.join(OUT, "*.npz"))):
        z = np.load(p)
        F, T = z["x"].shape
        coef = R.warp_coef(F, T, z["pt"], int(z["i"]), int(z["d"]), z["E"])
        got = R.spec_augment(z["x"], coef, z["fmask"], z["tmask"])
        fig[os.path.basename(p)[:-4]] = float(np.abs(got - z["out"]).max())
    with open(os.path.join(OUT, "reference_noise.json"), "w") as f:
        json.dump(fig, f, indent=1, sort_keys=True)
        f.write("\n")
    with open(os.path.join(OUT, "README.md"), "w") as f:
        f.write("# SpecAugment fixtures\n\nWritten by `tests/golden/make_spec_augment.py` from the reference's own `spec_augment` / "
                "`sparse_image_warp` (see its docstring for the contents of a file).\n\n`reference_noise.json` and the table "
                "below hold, per fixture, max |fp64 restatement - reference output| with the restatement of "
                "`tests/spec_augment_reference.py` run from the recorded draws: the fp32 noise of the reference itself, and the "
                "yardstick of `tests/test_gpu_spec_augment.py`.\n\n| fixture | F | T | max abs difference |\n|---|---|---|---|\n")
        for name in sorted(fig):
            F, T = np.load(os.path.join(OUT, name + ".npz"))["x"].shape
            f.write("| %s | %d | %d | %.3e |\n" % (name, F, T, fig[name]))


if __name__ == "__main__":
    main()
