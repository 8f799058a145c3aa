"""Loading of the golden fixtures (tests/golden/*.npz, produced by tests/golden/make_golden.py from the real
reference) and regeneration of their inputs/parameters from the stored seeds."""
import glob
import json
import os

import numpy as np
import torch

from deepspeech.pytorch_amd import synth

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- helpers of the kernel-level GPU tests (test_gpu_kernels.py, test_gpu_norm.py, test_gpu_seqops.py) -------------------------
DEV = "cuda"


def cu(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype).contiguous()


def rnd(a, dtype):
    """what the device sees after storing `a` in `dtype` (numpy float64 in, float64 out)"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(torch.float64).numpy()


def np64(t):
    return t.detach().to(torch.float64).cpu().numpy()


def relerr(got, ref):
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)


# fp32 storage: tight (the 1e-3 north-star bar with margin); bf16 storage: rounding of the stored outputs (2^-8 relative) plus
# accumulation noise
TOL = {torch.float32: 2e-5, torch.bfloat16: 1.2e-2}


def fixture_names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))


# Golden cases the whole-class GPU tests skip: none.  (rnn_bi_1024 was parked in round 1: on the GPU its conv1 weight gradient
# is 2.513e-3 of its scale away from the reference because ONE pre-Hardtanh value of the second conv block is 5.5e-7 from the
# clamp boundary 0 -- inside fp32 rounding of the BatchNorm output -- and Hardtanh's gradient is discontinuous there
# (tests/test_oracle_vs_golden.py::test_hardtanh_boundary_flip_explains_...).  check_grads_or_flip_variant below accepts the
# reference gradient or ONE consistent flip variant for such a case and reports which.)
GPU_PENDING = ()


def gpu_fixture_names():
    return [n for n in fixture_names() if n not in GPU_PENDING]


class Fixture:
    def __init__(self, name):
        self.name = name
        self.z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
        self.meta = json.loads(bytes(self.z["meta_json"]).decode())
        m = self.meta
        self.cfg = dict(rnn_type=m["rnn_type"], hidden_size=m["hidden_size"], hidden_layers=m["hidden_layers"],
                        bidirectional=m["bidirectional"], lookahead_context=m.get("lookahead_context", 20))
        self.lengths = np.asarray(m["lengths"], dtype=np.int64)
        self.sample_rate = m.get("sample_rate", 16000)      # SpectConfig.sample_rate: 161 frequency bins at 16 kHz, 81 at 8 kHz
        self.labels = m.get("labels") or (["_", "'"] + [chr(ord("A") + i) for i in range(26)] + [" "])   # reference labels.json

    def batch(self):
        m = self.meta
        inputs, targets, pct, tsz = synth.synth_batch(self.lengths, m["data_seed"],
                                                      chars_per_second=m.get("chars_per_second", 12.0), n_labels=m.get("n_labels", 29),
                                                      n_freq=m.get("sample_rate", 16000) // 100 + 1)
        if "long_target_sample" in m:
            i = m["long_target_sample"]
            rs = np.random.RandomState(m["data_seed"] + 999)
            tsz = tsz.copy()
            parts, off = [], 0
            for j, s in enumerate(tsz):
                if j == i:
                    parts.append(rs.randint(1, 29, size=int(self.lengths[i])).astype(np.int64))
                else:
                    parts.append(targets[off:off + s])
                off += s
            tsz[i] = int(self.lengths[i])
            targets = np.concatenate(parts)
        return inputs, targets, pct, tsz

    def params(self):
        m = self.meta
        P = synth.synth_params({k: tuple(v) for k, v in m["shapes"].items()}, m["param_seed"])
        g = m.get("bn_gain")
        if g:
            for k in ("conv.seq_module.1.weight", "conv.seq_module.4.weight"):
                P[k] = (P[k] * g).astype(np.float32)
        return P

    def grad_names(self):
        return sorted(k.split(".", 1)[1] for k in self.z.files if k.startswith("grad.") or k.startswith("gradsub."))

    def rel_l2(self, name, g, which="grad"):
        """Relative L2 distance of gradient `g` (full array) from the stored reference gradient (on the stored sub-sample for
        big tensors).  which: "grad" = the reference run in float64, "grad_ac" = the reference under autocast(bfloat16)."""
        g = np.asarray(g, dtype=np.float64)
        sub = which.replace("grad", "gradsub")
        if which + "." + name in self.z.files:
            ref = self.z[which + "." + name].astype(np.float64)
            got = g.reshape(ref.shape)
        else:
            ref = self.z[sub + "." + name].astype(np.float64)
            got = g.reshape(-1)[::self.meta["stride"]]
        return float(np.sqrt(((got - ref) ** 2).sum()) / max(np.sqrt((ref ** 2).sum()), 1e-30))

    def check_grad(self, name, g, rtol, atol_scale=1.0):
        """Compare gradient `g` (full array) with the stored reference gradient. Returns max abs err / scale."""
        g = np.asarray(g, dtype=np.float64)
        if "grad." + name in self.z.files:
            ref = self.z["grad." + name].astype(np.float64)
            got = g.reshape(ref.shape)
        else:
            ref = self.z["gradsub." + name].astype(np.float64)
            got = g.reshape(-1)[::self.meta["stride"]]
            l2 = float(self.z["gradl2." + name])
            assert abs(np.sqrt((g ** 2).sum()) - l2) <= rtol * max(l2, 1e-3) * 4, (name, "l2 norm")
        # floor: gradients that are exactly 0 in exact arithmetic (conv bias in front of BatchNorm when nothing
        # is masked) are pure rounding noise in any implementation
        scale = max(np.abs(ref).max(), 1e-3) * atol_scale
        err = np.abs(got - ref).max() / scale
        assert err <= rtol, "grad %s: max err %.3e of scale %.3e (rel %.3e > %.1e)" % (
            name, np.abs(got - ref).max(), scale, err, rtol)
        return err


def hardtanh_flip_variants(fx, thresh=2e-6, max_elems=3):
    """Gradients of every parameter (oracle, float64) with the Hardtanh decisions of the boundary-degenerate
    pre-activations flipped.  The reference function's gradient is discontinuous where a pre-Hardtanh value equals a clamp
    boundary (model.py:160,163,192: Hardtanh(0, 20)); an element closer to it than fp32 rounding of the BatchNorm output
    (a few 1e-7 at unit scale) can legitimately fall on either side in any fp32 implementation, the reference's own
    included.  Returns [dict(name -> grad)] for every non-empty subset of the (at most max_elems) elements within `thresh`
    of a boundary; empty when the case has none."""
    import itertools
    from oracle import ds2_oracle as O
    P = {k: v.astype(np.float64) for k, v in fx.params().items()}
    inputs, targets, pct, tsz = fx.batch()
    sizes = O.input_sizes_from_percentages(pct, inputs.shape[3])
    out, out_lens, _, cache = O.model_forward(P, fx.cfg, inputs.astype(np.float64), sizes, train=True)
    lp = O.log_softmax(cache["logits_tnc"])
    loss, nll, dlp = O.ctc_loss_and_grad_fast(lp, targets, out_lens, tsz, blank=0)
    dlogits = dlp - np.exp(lp) * dlp.sum(-1, keepdims=True)
    sites = []                                           # (array, index, boundary)
    planes = [(cache["conv"]["z1"], ~cache["conv"]["m1"]), (cache["conv"]["z2"], ~cache["conv"]["m2"])]
    if "la_pre" in cache:
        planes.append((cache["la_pre"], np.ones(cache["la_pre"].shape, dtype=bool)))
    for z, valid in planes:
        for b in (O.HT_MIN, O.HT_MAX):
            near = valid & (np.abs(z - b) < thresh)
            for idx in zip(*np.nonzero(near)):
                sites.append((z, idx, float(b)))
    sites = sorted(sites, key=lambda s_: abs(s_[0][s_[1]] - s_[2]))[:max_elems]
    variants = []
    for r in range(1, len(sites) + 1):
        for subset in itertools.combinations(sites, r):
            old = [z[idx] for z, idx, b in subset]
            for z, idx, b in subset:
                z[idx] = 2.0 * b - z[idx]               # reflect across the boundary: the other Hardtanh decision
            variants.append(O.model_backward(P, fx.cfg, cache, dlogits))
            for (z, idx, b), o in zip(subset, old):
                z[idx] = o
    return variants


def check_grads_or_flip_variant(fx, grads, rtol_of):
    """grads: name -> full gradient array of the implementation under test; rtol_of(name) -> bar relative to the tensor's
    max.  Passes if every gradient matches the stored reference gradient, or -- for a boundary-degenerate case -- one and
    the same flip variant of hardtanh_flip_variants.  Returns "reference" or "flip-variant"."""
    try:
        for k, g in grads.items():
            fx.check_grad(k, g, rtol=rtol_of(k))
        return "reference"
    except AssertionError as first:
        for v in hardtanh_flip_variants(fx):
            ok = True
            for k, g in grads.items():
                ref = np.asarray(v[k], dtype=np.float64)
                scale = max(np.abs(ref).max(), 1e-3)
                if np.abs(np.asarray(g, dtype=np.float64).reshape(ref.shape) - ref).max() / scale > rtol_of(k):
                    ok = False
                    break
            if ok:
                return "flip-variant"
        raise first


def check_persist_routing(answer, covered):
    """Compares a routing of the persistent recurrent sweeps with the recorded table tests/golden/routing/persist_routing.npz (written by
    tests/golden/make_persist_routing.py from the parent of the routing refactor, on an MI355X), row by row.
    answer(dtype, cell, D, N, H, variant) -> (supported, kind, ws_bytes); covered(dtype, cell, D, N, H) -> shape_covered.
    Of the recorded variants only the columns of the live routing bits are compared (0, 1, 8, 16 for bf16; 0, 1 for fp32): the bits
    2, 32, 64 and 128 of the recording are retired and a variant that carries one is refused.  Returns the number of rows compared."""
    z = np.load(os.path.join(GOLDEN_DIR, "routing", "persist_routing.npz"))
    assert b"recorded from commit 35ac4a121fe5370703d8e3e01c8a6a90900492fd" in bytes(z["header"]) and b"does NOT" not in bytes(z["header"])
    Hs, Ns, variants = z["H"].tolist(), z["N"].tolist(), z["variants"].tolist()
    assert Hs == list(range(16, 1601, 16)) and len(Ns) == 90 and variants == [0, 1, 2, 8, 16, 32, 64, 128]
    rows, bad = 0, []
    for name, dtype, vs, live in (("bf16", 1, variants, (0, 1, 8, 16)), ("f32", 0, variants[:2], (0, 1))):
        sup, kind, ws, cov = (z["%s_%s" % (name, k)] for k in ("supported", "kind", "ws", "covered"))
        assert sup.shape == (3, 2, len(Hs), len(Ns), len(vs)) and cov.shape == sup.shape[:4]
        columns = [(vs.index(v), v) for v in live]
        for cell in range(3):
            for D in (1, 2):
                for hi, H in enumerate(Hs):
                    for ni, N in enumerate(Ns):
                        if int(covered(dtype, cell, D, N, H)) != cov[cell, D - 1, hi, ni]:
                            bad.append((name, cell, D, N, H, "covered"))
                        for vi, v in columns:
                            got = tuple(int(x) for x in answer(dtype, cell, D, N, H, v))
                            want = (int(sup[cell, D - 1, hi, ni, vi]), int(kind[cell, D - 1, hi, ni, vi]), int(ws[cell, D - 1, hi, ni, vi]))
                            rows += 1
                            if got != want:
                                bad.append((name, cell, D, N, H, v, got, want))
    assert not bad, "%d rows differ from the recorded routing, first: %s" % (len(bad), bad[:5])
    return rows
