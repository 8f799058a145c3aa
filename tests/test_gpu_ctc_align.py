"""GPU checks of CTC forced alignment (ds2_ctc_align, ops.ctc_align, align.ForcedAligner, tools/align.py) against the fp64
restatement tests/ctc_align_reference.py.

Exact cases: log-probabilities are multiples of 1/8 in [-12, 0], so every fp32 sum of up to T' <= 2100 of them is exact
(T' * 12 * 8 < 2^24) and the device must equal the restatement BIT FOR BIT, ties included: frame_state, tok_start, tok_end,
tok_logp and score.  Modes 0 / 1 (logits, probabilities) go through fp32 transcendental functions: there the device path must be
a valid alignment and its score within the bound tests/test_gpu_kernels.py::_ctc_check puts on the per-sample nll."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import ctc_align_reference as R
from fixtures import DEV, Fixture
from oracle import ds2_oracle as O

pytestmark = pytest.mark.gpu

WG = 256                    # workgroup of k_ctc_align (AL_THREADS in csrc/ds2_align.hip): thread j owns states j, j + WG, ...
SENTINEL = 0x7B7B7B7B
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ops():
    from deepspeech.pytorch_amd import ops as _ops
    return _ops


def nll_bound(ref):
    """the bar of _ctc_check (tests/test_gpu_kernels.py) on a per-sample nll: np.allclose(got, ref, rtol=2e-5, atol=1e-4)"""
    return 1e-4 + 2e-5 * abs(ref)


def _target(rs, L, C, blank, repeats):
    """L labels that avoid the blank; repeats: 0 = no adjacent equal labels, k > 0 = exactly k adjacent equal pairs (at the front),
    -1 = one label throughout"""
    pool = [c for c in range(C) if c != blank]
    t = np.empty(L, dtype=np.int64)
    for i in range(L):
        if repeats == -1 and i > 0:
            t[i] = t[0]
        elif i > 0 and i <= repeats:
            t[i] = t[i - 1]
        else:
            t[i] = pool[rs.randint(len(pool))]
            while i > 0 and t[i] == t[i - 1]:
                t[i] = pool[rs.randint(len(pool))]
    return t


def n_repeats(t):
    return int((t[1:] == t[:-1]).sum()) if len(t) > 1 else 0


@functools.lru_cache(maxsize=None)
def _exact_case(spec, C, blank, seed):
    """spec: tuple of clips (L, T, repeats), T = frames or a string 'L', 'L+r-1', 'L+r' resolved on the target.  Returns
    (lps [list of (T, C) float64], targets, sizes, references): computed once, shared by the layouts."""
    rs = np.random.RandomState(seed)
    lps, targets, sizes, refs = [], [], [], []
    for L, T, repeats in spec:
        t = _target(rs, L, C, blank, repeats)
        r = n_repeats(t)
        T = {"L": L, "L+r-1": L + r - 1, "L+r": L + r}.get(T, T)
        T = max(int(T), 0)
        lp = rs.randint(-96, 1, size=(T, C)) / 8.0
        lps.append(lp)
        targets.append(t)
        sizes.append(T)
        refs.append(R.align(lp, t, blank))
    return lps, targets, sizes, refs


def _device_input(lps, sizes, Tp, C, layout):
    """(N, Tp, C) device tensor holding clip n's rows in its first sizes[n] frames and NaN elsewhere (nothing beyond a clip's own
    frames may be read).  layout 'rows': the transpose view of the head's [Tp*N][ld] rows; 'contig': a contiguous tensor."""
    N = len(lps)
    host = np.full((N, Tp, C), np.nan, dtype=np.float32)
    for n, lp in enumerate(lps):
        host[n, :sizes[n]] = lp
    if layout == "contig":
        return torch.from_numpy(host).to(DEV)
    ld = (C + 31) // 32 * 32
    rows = torch.full((Tp * N, ld), float("nan"), dtype=torch.float32, device=DEV)
    rows.view(Tp, N, ld)[:, :, :C] = torch.from_numpy(host).to(DEV).transpose(0, 1)
    x = rows.view(Tp, N, ld)[:, :, :C].transpose(0, 1)
    assert x.stride() == (ld, N * ld, 1)
    return x


def _check_exact(got, targets, sizes, refs, Tp):
    fs, ts, te, tl, score = [g.cpu().numpy() for g in got]
    assert fs.dtype == np.int32 and tl.dtype == np.float32 and score.dtype == np.float32
    off = 0
    for n, ref in enumerate(refs):
        L, T = len(targets[n]), sizes[n]
        assert score[n] == np.float32(ref.score), (n, score[n], ref.score)
        assert np.array_equal(fs[n, :T], ref.frame_state), (n, fs[n, :T], ref.frame_state)
        assert np.all(fs[n, T:] == -1), n
        assert np.array_equal(ts[off:off + L], ref.tok_start) and np.array_equal(te[off:off + L], ref.tok_end), n
        assert np.array_equal(tl[off:off + L], ref.tok_logp.astype(np.float32)), n
        off += L
    assert off == len(ts) == len(te) == len(tl)


def _run_exact(spec, C, blank, layout, seed, extra_pad=3, max_target_len=None):
    lps, targets, sizes, refs = _exact_case(spec, C, blank, seed)
    Tp = max(max(sizes), 1) + extra_pad
    x = _device_input(lps, sizes, Tp, C, layout)
    flat = np.concatenate(targets).astype(np.int32) if targets else np.zeros(0, np.int32)
    got = ops().ctc_align(x, torch.tensor(sizes, dtype=torch.int32), torch.from_numpy(flat),
                          torch.tensor([len(t) for t in targets], dtype=torch.int32), blank=blank, mode="log_probs",
                          max_target_len=max_target_len)
    _check_exact(got, targets, sizes, refs, Tp)
    return refs


CLASSES = [(29, 0, "rows"), (300, 299, "contig"), (29, 0, "contig"), (300, 299, "rows")]
EXACT = {
    # around one wave of states: S = 1, 3, 5, 63, 65, 67 with room for blanks
    "wave_edges": tuple((L, 2 * L + 3, 0) for L in (0, 1, 2, 31, 32, 33)),
    # T' = 1, 2, L (a path without a blank), and with adjacent equal labels L + repeats - 1 (infeasible) / L + repeats (tightest)
    "frame_edges": ((1, 1, 0), (2, 1, 0), (0, 1, 0), (1, 2, 0), (2, 2, 0), (2, 2, 1), (3, 2, 0), (5, "L", 0), (33, "L", 0),
                    (5, "L+r-1", 2), (5, "L+r", 2), (33, "L+r-1", 3), (33, "L+r", 3), (32, "L+r", 1)),
    # one label throughout: every label needs its blank
    "one_label": ((4, "L+r-1", -1), (4, "L+r", -1), (4, 12, -1), (40, "L+r-1", -1), (40, "L+r", -1), (40, 100, -1)),
    # thread-map edges of the workgroup: S = WG - 1 is the most one pass holds (S is odd), S = WG + 1 needs a second pass of one state
    "wg_minus_1": ((WG // 2 - 1, WG + 10, 2), (3, 9, 1)),
    "wg_plus_1": ((WG // 2, WG + 10, 2), (3, 9, 1)),
    "two_passes_full": ((WG - 1, 2 * WG + 7, 1), (WG // 2, WG, 0)),           # S = 2 WG - 1
    "three_passes": ((WG, 2 * WG + 7, 1), (7, 30, 0)),                        # S = 2 WG + 1: a third pass of one state
    "four_passes_full": ((2 * WG - 1, 4 * WG + 5, 2), (WG, "L+r", 0)),        # S = 4 WG - 1
    "five_passes": ((2 * WG, 4 * WG + 5, 2), (1, 3, 0)),                      # S = 4 WG + 1: the widest thread map, barely used
}


@pytest.mark.parametrize("C,blank,layout", CLASSES)
@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_cases_equal_the_restatement_bit_for_bit(name, C, blank, layout):
    refs = _run_exact(EXACT[name], C, blank, layout, seed=len(name) + C)
    if name == "frame_edges":
        feas = [r.score > -np.inf for r in refs]
        assert feas == [True, False, True, True, True, False, False, True, True, False, True, False, True, True]
        assert list(refs[7].frame_state) == [1, 3, 5, 7, 9]                   # T' = L: no blank at all
    if name == "one_label":
        assert [r.score > -np.inf for r in refs] == [False, True, True, False, True, True]


@pytest.mark.parametrize("spec", [((0, 7, 0),), ((0, 7, 0), (0, 3, 0)), ((0, 0, 0),)])
@pytest.mark.parametrize("layout", ["rows", "contig"])
def test_batches_without_any_label(spec, layout):
    """every target of the call is empty (no targets at all): the all-blank path for every clip with frames"""
    refs = _run_exact(spec, 29, 0, layout, seed=1)
    for (L, T, _), r in zip(spec, refs):
        assert list(r.frame_state) == [0] * T and (r.score > -np.inf) == (T > 0)


@pytest.mark.parametrize("max_target_len", [300, 600, 2047])
def test_small_clips_under_every_thread_map(max_target_len):
    """max_target_len selects the thread map (states per thread) for the whole launch: short clips give the same result under the
    wider ones"""
    _run_exact(EXACT["wave_edges"] + EXACT["frame_edges"], 29, 0, "rows", seed=5, max_target_len=max_target_len)


def test_longest_target():
    """2047 labels (the cap: S = 4095 states, 16 per thread) on 2100 frames, and a second clip that ends inside the first
    trace-back window"""
    _run_exact(((2047, 2100, 3), (20, 41, 1)), 29, 0, "rows", seed=2047, extra_pad=1)


def test_beyond_the_cap_is_refused():
    o = ops()
    x = torch.zeros((1, 8, 29), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="2047"):
        o.ctc_align(x, [8], np.ones(2048, np.int32), [2048], mode="log_probs")
    from deepspeech.pytorch_amd import _lib
    assert _lib.query("ds2_ctc_align_ws_bytes", 8, 1, 2048) == -1
    d = torch.zeros(8, dtype=torch.int32, device=DEV)
    rc = _lib.load().ds2_ctc_align(o.P(x), 8 * 29, 29, 1, 8, 29, 2, o.P(d), o.P(d), o.P(d), o.P(d), 2048, 0, o.P(d), o.P(d), o.P(d),
                                   o.P(x), o.P(x), o.P(x), o.S())
    assert rc == 1002                                                          # DS2_ERR_ARG, nothing launched


@pytest.mark.parametrize("C,blank,layout", CLASSES[:2])
def test_mixed_batch_writes_every_output_element(C, blank, layout):
    """N = 5 clips of different sizes and target lengths in one launch, one without frames and one without labels, Tp beyond every
    size, outputs pre-filled with a sentinel: everything is written, frames beyond a clip's size are -1"""
    from deepspeech.pytorch_amd import _lib
    o = ops()
    spec = ((9, 40, 1), (3, 0, 0), (0, 17, 0), (30, 29, 0), (70, 150, 2))       # sizes 40, 0, 17, 29 (infeasible), 150
    lps, targets, sizes, refs = _exact_case(spec, C, blank, 77)
    N, Tp = 5, 170
    x = _device_input(lps, sizes, Tp, C, layout)
    tl = [len(t) for t in targets]
    total, maxl = sum(tl), max(tl)
    i32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=DEV)      # noqa: E731
    fs = torch.full((N, Tp), SENTINEL, dtype=torch.int32, device=DEV)
    ts, te = torch.full((total,), SENTINEL, dtype=torch.int32, device=DEV), torch.full((total,), SENTINEL, dtype=torch.int32, device=DEV)
    tlp = torch.full((total,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    score = torch.full((N,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    ws = torch.empty(_lib.query("ds2_ctc_align_ws_bytes", Tp, N, maxl), dtype=torch.uint8, device=DEV)
    offs = np.concatenate([[0], np.cumsum(tl)[:-1]])
    szd, tgd, offd, tld = i32(sizes), i32(np.concatenate(targets)), i32(offs), i32(tl)      # (alive until the launch has run)
    _lib.call("ds2_ctc_align", o.P(x), x.stride(0), x.stride(1), N, Tp, C, 2, o.P(szd), o.P(tgd), o.P(offd), o.P(tld), maxl, blank,
              o.P(fs), o.P(ts), o.P(te), o.P(tlp), o.P(score), o.P(ws), o.S())
    for t in (fs, ts, te, tlp.view(torch.int32), score.view(torch.int32)):
        assert not bool((t == SENTINEL).any())
    _check_exact((fs, ts, te, tlp, score), targets, sizes, refs, Tp)
    assert [r.score > -np.inf for r in refs] == [True, False, True, False, True]
    assert bool((fs[1] == -1).all()) and bool((fs[3] == -1).all()) and float(score[1]) == float("-inf")


# ---- modes 0 and 1: random logits and their softmax ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _soft_case(Tp, C, blank):
    rs = np.random.RandomState(Tp + C)
    sizes, tlens = ([50, 49, 33, 20], [20, 7, 16, 0]) if Tp == 50 else ([333, 300, 251, 200], [120, 17, 99, 1])
    logits = (rs.standard_normal((4, Tp, C)) * 2).astype(np.float32)
    targets = [_target(rs, L, C, blank, 2 if L > 3 else 0) for L in tlens]
    l64 = logits.astype(np.float64)
    probs = np.exp(O.log_softmax(l64)).astype(np.float32)
    lp_of = {"logits": O.log_softmax(l64), "probs": np.log(probs.astype(np.float64))}      # what the device is given, in float64
    refs = {k: [R.align(lp[n, :sizes[n]], targets[n], blank) for n in range(4)] for k, lp in lp_of.items()}
    return logits, probs, targets, sizes, lp_of, refs


@pytest.mark.parametrize("kind", ["logits", "probs"])
@pytest.mark.parametrize("Tp,C,blank,layout", [(50, 29, 0, "rows"), (333, 29, 0, "rows"), (333, 29, 0, "contig"), (50, 300, 299, "contig"),
                                               (333, 300, 299, "rows")])
def test_logits_and_probabilities(Tp, C, blank, layout, kind):
    logits, probs, targets, sizes, lp_of, refs = _soft_case(Tp, C, blank)
    src = logits if kind == "logits" else probs
    x = _device_input([src[n, :sizes[n]] for n in range(4)], sizes, Tp, C, layout)
    flat = np.concatenate(targets).astype(np.int32)
    tl = [len(t) for t in targets]
    run = lambda: ops().ctc_align(x, torch.tensor(sizes), torch.from_numpy(flat), torch.tensor(tl), blank=blank, mode=kind)   # noqa: E731
    got = run()
    fs, ts, te, tlp, score = [g.cpu().numpy() for g in got]
    off = 0
    for n in range(4):
        T, L, ref, lp = sizes[n], tl[n], refs[kind][n], lp_of[kind][n, :sizes[n]]
        assert R.collapses_to(fs[n, :T], targets[n], blank) and np.all(fs[n, T:] == -1)
        own = R.rescore(lp, fs[n, :T], targets[n], blank)
        print("clip %d: device %.6f, its path in float64 %.6f, optimum %.6f (bound %.2e)" % (n, score[n], own, ref.score, nll_bound(ref.score)))
        assert abs(score[n] - own) <= nll_bound(own) and abs(score[n] - ref.score) <= nll_bound(ref.score)
        for i in range(L):                                                     # spans and label sums describe the device's own path
            fr = np.nonzero(fs[n, :T] == 2 * i + 1)[0]
            assert (ts[off + i], te[off + i]) == (fr[0], fr[-1]) and np.array_equal(fr, np.arange(fr[0], fr[-1] + 1))
            want = lp[fr, targets[n][i]].sum()
            assert abs(tlp[off + i] - want) <= nll_bound(want)
        off += L
    # repeatability: the same bits on a second launch
    for a, b in zip(got, run()):
        assert torch.equal(a, b)


def test_best_path_against_the_loss_kernel():
    """score <= -nll of ds2_ctc_loss_grad on the same logits (the best path is one term of the likelihood); and when the logits put
    all but 1e-6 of the mass on one path, the two agree"""
    o = ops()
    logits, _, targets, sizes, _, _ = _soft_case(333, 29, 0)
    N, Tp, C = 5, 333, 29
    tl = [len(t) for t in targets] + [40]
    # clip 4: one path with all but 1e-6 of the mass -- per frame 1 - d on the path's label, d = 1e-6 / T'
    rs = np.random.RandomState(4)
    peaked_t = _target(rs, 40, C, 0, 2)
    path = np.repeat(R.extended(peaked_t, 0)[:-1], 4)[:Tp]                      # blank x4, label x4, ... : 320 frames
    path = np.concatenate([path, np.zeros(Tp - len(path), dtype=np.int64)])
    gap = np.log((1 - 1e-6 / Tp) * (C - 1) / (1e-6 / Tp))
    peaked = np.zeros((Tp, C), dtype=np.float32)
    peaked[np.arange(Tp), path] = gap
    all_logits = np.concatenate([logits, peaked[None]], 0)
    sizes = list(sizes) + [Tp]
    rows = torch.zeros((Tp * N, 32), dtype=torch.float32, device=DEV)
    rows.view(Tp, N, 32)[:, :, :C] = torch.from_numpy(all_logits).to(DEV).transpose(0, 1)
    flat = torch.from_numpy(np.concatenate(list(targets) + [peaked_t]).astype(np.int32)).to(DEV)
    tld = torch.tensor(tl, dtype=torch.int32, device=DEV)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(tl)[:-1]]), dtype=torch.int32, device=DEV)
    szd = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    _, nll, _ = o.ctc_loss_grad(rows, flat, offs, szd, tld, Tp, N, C, 0, max(tl))
    x = rows.view(Tp, N, 32)[:, :, :C].transpose(0, 1)
    fs, _, _, _, score = o.ctc_align(x, szd, flat, tld, blank=0, mode="logits", max_target_len=max(tl))     # lengths on the device
    nll, score = nll.cpu().numpy().astype(np.float64), score.cpu().numpy().astype(np.float64)
    print("score", score, "-nll", -nll)
    for n in range(N):
        assert (nll[n] > 0 or n == 4) and score[n] <= -nll[n] + nll_bound(nll[n])      # (nll 0 = the loss found no path)
    assert abs(score[4] + nll[4]) <= nll_bound(nll[4])
    assert np.array_equal(R.extended(peaked_t, 0)[fs[4].cpu().numpy()], path)


# ---- the class and the tool --------------------------------------------------------------------------------------------------
def _argmax_pattern_probs(rs, pattern, C):
    p = rs.uniform(0.1, 1.0, size=(len(pattern), C))
    p[np.arange(len(pattern)), pattern] = 3.0
    return (p / p.sum(-1, keepdims=True)).astype(np.float32)


def test_forced_aligner_end_to_end_on_a_model():
    """A tiny model (the gru_bi_tiny fixture: its configuration and weights) in eval mode, aligned with its own greedy transcripts.
    The arg-max path is the best path over ALL label sequences, so it is the best path of its own transcript; it is the only one --
    and frame_labels must equal the arg-max frames whatever the tie rule -- when no frame's two highest probabilities are close:
    another path differs in at least one frame and loses log(p1 / p2) >= (p1 - p2) / p1 >= 1e-4 there, far above the fp32 error
    of a sum of <= 31 log-probabilities of magnitude <= 4 (31 * 4 * 6e-8 = 7e-6).  Every clip whose smallest gap p1 - p2 exceeds
    1e-4 is held to that (data seed 6: on the CPU oracle the three clips' smallest gaps are 7.9e-4, 1.5e-3 and 3.5e-4, every
    one at least 3.5 times the threshold).  This set
    contains every clip without adjacent equal labels in its arg-max frames (and without ties); the fixture's weights emit one label
    over long runs, so the check below adds a constructed output without such runs."""
    from test_gpu_model import build
    from deepspeech.pytorch_amd import synth
    from deepspeech.pytorch_amd.align import ForcedAligner
    fx = Fixture("gru_bi_tiny")
    m = build(fx, 32).eval()
    inputs, _, pct, _ = synth.synth_batch(fx.lengths, 6)
    with torch.no_grad():
        out, out_sizes, _ = m(torch.from_numpy(inputs).to(DEV), torch.from_numpy(pct.copy()).mul_(int(inputs.shape[3])).int())
    strings, _ = m.evaluation_decoder.decode(out, out_sizes)
    aligner = ForcedAligner.from_model(m)
    assert aligner.frame_seconds == 0.02
    als = aligner.align(out, out_sizes, transcripts=[s[0] for s in strings], kind="probs")
    top2 = out.topk(2, dim=-1).values.cpu()
    arg = out.argmax(-1).cpu()
    qualified = 0
    for n, a in enumerate(als):
        T = int(out_sizes[n])
        if strings[n][0]:
            assert a.feasible and a.frames == T and len(a.chars) == len(strings[n][0])
            assert ''.join(c.text for c in a.chars) == strings[n][0]
            assert ' '.join(w.text for w in a.words) == ' '.join(strings[n][0].split())
        if float((top2[n, :T, 0] - top2[n, :T, 1]).min()) > 1e-4:
            qualified += 1
            assert torch.equal(a.frame_labels.long(), arg[n, :T])
            assert abs(a.score - float(out[n, :T].max(-1).values.log().double().sum())) <= nll_bound(a.score)
    assert qualified >= 1
    # a constructed output whose arg-max frames have no two equal labels adjacent: "A_BC__D A"
    labels = aligner.labels
    pattern = [labels.index(c) for c in "A_BC__D A"]
    probs = torch.from_numpy(_argmax_pattern_probs(np.random.RandomState(0), pattern, len(labels)))[None].to(DEV)
    (a,) = aligner.align(probs, [len(pattern)], transcripts=["ABCD A"])
    assert a.feasible and a.frame_labels.tolist() == pattern
    assert [c[:3] for c in a.chars] == [("A", 0, 0), ("B", 2, 2), ("C", 3, 3), ("D", 6, 6), (" ", 7, 7), ("A", 8, 8)]
    assert [(w.text, w.start_frame, w.end_frame) for w in a.words] == [("ABCD", 0, 6), ("A", 8, 8)]
    assert (a.words[0].start_s, a.words[0].end_s) == (0.0, 7 * 0.02)
    assert ForcedAligner.flag([a], -50.0) == [] and ForcedAligner.flag([a], 0.0) == [0]
    (empty,) = aligner.align(probs, [len(pattern)], transcripts=[""])          # a batch without any label: the all-blank path
    assert empty.feasible and empty.chars == [] and empty.words == [] and empty.frame_labels.tolist() == [0] * len(pattern)
    (bad,) = aligner.align(probs[:, :3], [3], transcripts=["ABCD A"])           # six labels on three frames
    assert not bad.feasible and bad.chars == [] and bad.frame_labels.tolist() == [-1, -1, -1] and ForcedAligner.flag([bad], -1e9) == [0]


def test_tool_reproduces_the_class(tmp_path):
    from deepspeech.pytorch_amd.align import ForcedAligner
    from deepspeech.pytorch_amd.configs import LABELS
    rs = np.random.RandomState(11)
    sents = ["HELLO  WORLD", " A'B", "", "TOO LONG FOR TWO FRAMES"]
    sizes = np.array([40, 9, 5, 2], dtype=np.int32)
    probs = rs.dirichlet(np.ones(len(LABELS)) * 0.3, size=(4, 40)).astype(np.float32)
    targets = np.array([LABELS.index(c) for s in sents for c in s], dtype=np.int32)
    npz = str(tmp_path / "batch.npz")
    np.savez(npz, probs=probs, sizes=sizes, targets=targets, target_sizes=np.array([len(s) for s in sents], dtype=np.int32))
    spec = importlib.util.spec_from_file_location("align_tool", os.path.join(ROOT, "tools", "align.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = str(tmp_path / "align.json")
    tool.main([npz, "--output-path", out, "--frame-seconds", "0.04", "--min-mean-logp", "-3.0"])
    with open(out) as f:
        res = json.load(f)
    als = ForcedAligner(LABELS, blank_index=LABELS.index('_'), frame_seconds=0.04).align(torch.from_numpy(probs).to(DEV), sizes,
                                                                                         transcripts=sents)
    assert len(res["clips"]) == 4 and [c["feasible"] for c in res["clips"]] == [True, True, True, False]
    for c, a in zip(res["clips"], als):
        assert c["feasible"] == a.feasible and c["frames"] == a.frames and (c["score"] == a.score if a.feasible else c["score"] is None)
        assert [(w["word"], w["start_frame"], w["end_frame"], w["start_s"], w["end_s"], w["logp"]) for w in c["words"]] == [(w.text, w.start_frame, w.end_frame, w.start_s, w.end_s, w.logp) for w in a.words]
    assert [w["word"] for w in res["clips"][0]["words"]] == ["HELLO", "WORLD"] and [w["word"] for w in res["clips"][1]["words"]] == ["A'B"]
    assert res["flagged"] == ForcedAligner.flag(als, -3.0) and 3 in res["flagged"]
