"""GPU checks of the device CTC prefix beam search (ds2_beam_decode, ops.beam_decode, decoder.BeamCTCDecoder) against the numpy
restatement of its rules (tests/beam_reference.py, itself pinned by tests/test_beam_reference.py).

The kernel evaluates every log / exp in fp64 and rounds once to fp32, and the restatement in fp32 mode does the same, so the two
make the same selection at every step, exact fp32 ties included: the checks ask for identical label sequences, lengths and offsets
of all B beams.  (A skip rule on the selection-boundary gap would empty the grid: at T' = 200 the gap between the last kept and the
first dropped candidate is 1e-5 .. 1e-7 of the score, with exact ties at B >= 128.)  Only the order of output beams whose scores
are within 1e-6 of each other is compared as a set."""
import numpy as np
import pytest
import torch

from beam_reference import FLT_MIN, beam_search, brute_force
from fixtures import Fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _probs(rng, N, T, C, scale=3.0):
    z = rng.standard_normal((N, T, C)) * scale            # peaky rows, like the model's softmax outputs
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def _check(toks, offs, scores, p, sizes, blank, B, top_n, cutoff_prob):
    """kernel output of every utterance against the restatement; returns the restatement's results."""
    out = []
    for n in range(p.shape[0]):
        ref = beam_search(p[n], sizes[n], blank, B, top_n, cutoff_prob)
        rb = ref["beams"]
        alive = int(torch.isfinite(scores[n]).sum())
        assert alive == len(rb), (n, alive, len(rb))
        got = [(tuple(toks[n][b]), tuple(offs[n][b].tolist()), float(scores[n, b])) for b in range(alive)]
        for b in range(alive, B):
            assert toks[n][b] == [] and scores[n, b] == float("inf")
        assert len({g[0] for g in got}) == alive                               # never two equal strings
        # per string: offsets equal, score within 1e-4 relative (equal bits expected)
        gd, rd = {g[0]: g for g in got}, {r[0]: r for r in rb}
        assert set(gd) == set(rd), n
        for lab, (_, fr, s) in rd.items():
            assert gd[lab][1] == fr, (n, lab, gd[lab][1], fr)
            assert abs(gd[lab][2] - s) <= 1e-4 * max(1.0, abs(s)), (n, lab, gd[lab][2], s)
        # rank order: identical wherever adjacent scores are apart by more than 1e-6
        for b in range(alive):
            near = (b > 0 and rb[b][2] - rb[b - 1][2] <= 1e-6 * max(1.0, abs(rb[b][2]))) or \
                (b + 1 < alive and rb[b + 1][2] - rb[b][2] <= 1e-6 * max(1.0, abs(rb[b][2])))
            if not near:
                assert got[b][0] == rb[b][0], (n, b)
        out.append(ref)
    return out


def _sizes(rng, N, T):
    s = rng.integers(0, T + 1, size=N)
    if N >= 3:
        s[0], s[1] = T, 0
    else:
        s[0] = T
    return s.astype(np.int32)


# (N, T, C, B, cutoff_top_n, cutoff_prob, blank, strided (T, N, C) view)
GRID = [
    (1, 1, 5, 1, 40, 1.0, 0, False),
    (3, 2, 5, 2, 5, 1.0, 0, False),
    (3, 17, 29, 10, 40, 1.0, 0, True),
    (8, 17, 29, 128, 5, 0.9, 3, False),
    (8, 200, 29, 10, 40, 1.0, 0, True),
    (3, 200, 29, 128, 40, 0.9, 0, False),
    (1, 200, 29, 256, 40, 1.0, 0, False),
    (3, 17, 300, 10, 40, 1.0, 5, False),
    (3, 200, 5, 256, 5, 1.0, 0, False),
    (8, 17, 29, 2, 1, 1.0, 0, False),
    (3, 2, 29, 256, 40, 0.9, 28, True),
    (1, 17, 29, 256, 40, 1.0, 0, False),
]


@pytest.mark.parametrize("N,T,C,B,top_n,cutoff_prob,blank,strided", GRID)
def test_kernel_matches_restatement(N, T, C, B, top_n, cutoff_prob, blank, strided):
    from deepspeech.pytorch_amd import ops
    rng = np.random.default_rng(N * 1000 + T * 7 + C + B)
    p = _probs(rng, N, T, C)
    sizes = _sizes(rng, N, T)
    if strided:
        view = torch.from_numpy(np.ascontiguousarray(p.transpose(1, 0, 2))).to(DEV).transpose(0, 1)
        assert not view.is_contiguous()
    else:
        view = torch.from_numpy(p).to(DEV)
    toks, offs, scores = ops.beam_decode(view, torch.from_numpy(sizes), blank, B, top_n, cutoff_prob)
    assert scores.shape == (N, B) and len(toks) == N and all(len(t) == B for t in toks)
    _check(toks, offs, scores, p, sizes, blank, B, top_n, cutoff_prob)


def test_revived_prefixes_merge_by_string():
    """A prefix that was pruned and later re-created gets a new node while its surviving children hang off the old one; its
    extensions must still merge with those children.  Small beams over 64 seeds, where the restatement logs such merges."""
    from deepspeech.pytorch_amd import ops
    p = _probs(np.random.default_rng(33), 64, 40, 3, scale=1.0)
    sizes = np.full(64, 40, np.int32)
    toks, offs, scores = ops.beam_decode(torch.from_numpy(p).to(DEV), torch.from_numpy(sizes), 0, 3, 40, 1.0)
    refs = _check(toks, offs, scores, p, sizes, 0, 3, 40, 1.0)
    assert sum(r["revival_merges"] > 0 for r in refs) >= 5
    assert sum(r["revivals"] > 0 for r in refs) >= 20


@pytest.mark.parametrize("name", ["gru_bi_mid", "lstm_uni_la"])
def test_width_one_top_one_equals_greedy_decoder(name):
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder, GreedyDecoder
    fx = Fixture(name)
    probs = torch.from_numpy(fx.z["eval_probs"]).to(DEV)
    sizes = torch.from_numpy(fx.z["output_lengths"].copy())
    gs, go = GreedyDecoder(fx.labels).decode(probs, sizes)
    bs, bo = BeamCTCDecoder(fx.labels, beam_width=1, cutoff_top_n=1, cutoff_prob=1.0).decode(probs, sizes)
    assert [s[0] for s in bs] == [s[0] for s in gs] == fx.meta["transcripts"]
    for a, b in zip(bo, go):
        assert torch.equal(a[0], b[0])


def test_short_inputs_scores_equal_ctc_loss():
    """T' <= 6 with a beam wider than the number of prefixes and no pruning: every label string is a beam and its score is its
    CTC negative log-likelihood."""
    from deepspeech.pytorch_amd import ops
    N, T, C = 4, 6, 3
    p = _probs(np.random.default_rng(5), N, T, C, scale=1.0)
    toks, offs, scores = ops.beam_decode(torch.from_numpy(p).to(DEV), None, 0, 256, 40, 1.0)
    lp = torch.log(torch.from_numpy(p).double() + float(FLT_MIN))
    for n in range(N):
        alive = int(torch.isfinite(scores[n]).sum())
        assert {tuple(t) for t in toks[n][:alive]} == set(brute_force(p[n]))   # every string reachable in T' frames
        for b in range(alive):
            lab = toks[n][b]
            if lab:
                ref = float(torch.nn.functional.ctc_loss(lp[n][:, None, :], torch.tensor([lab]), torch.tensor([T]),
                                                         torch.tensor([len(lab)]), blank=0, reduction="none")[0])
            else:
                ref = -float(lp[n, :, 0].sum())
            assert abs(float(scores[n, b]) - ref) <= 1e-4 * max(1.0, ref), (n, lab, float(scores[n, b]), ref)


def test_two_runs_bit_identical():
    from deepspeech.pytorch_amd import ops
    p = torch.from_numpy(_probs(np.random.default_rng(9), 8, 200, 29)).to(DEV)
    sizes = torch.tensor([200, 150, 0, 199, 1, 77, 200, 31], dtype=torch.int32)
    a = ops.beam_decode(p, sizes, 0, 128, 40, 1.0)
    b = ops.beam_decode(p, sizes, 0, 128, 40, 1.0)
    assert a[0] == b[0] and torch.equal(a[2], b[2])
    assert all(torch.equal(x, y) for u, v in zip(a[1], b[1]) for x, y in zip(u, v))


def _edit(a, b):
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def _model(fx):
    from deepspeech.pytorch_amd import configs
    from deepspeech.pytorch_amd.model import DeepSpeech
    c = fx.cfg
    rt = getattr(configs.RNNType, c["rnn_type"])
    assert c["bidirectional"]
    mc = configs.BiDirectionalConfig(rnn_type=rt, hidden_size=c["hidden_size"], hidden_layers=c["hidden_layers"])
    m = DeepSpeech(labels=fx.labels, model_cfg=mc, precision=32, optim_cfg=configs.AdamConfig(),
                   spect_cfg=configs.SpectConfig(sample_rate=fx.sample_rate))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in fx.params().items()}, strict=True)
    return m.to(DEV)


def test_validation_step_with_beam_decoder():
    """attach_evaluation(BeamCTCDecoder(...)) with metrics that decode through it (targets through the greedy decoder's
    convert_to_strings, as the reference's test.py does); the WER / CER validation_step logs equal a computation of the test's
    own from the top beams."""
    from deepspeech.pytorch_amd import decoder as D
    fx = Fixture("gru_bi_mid")
    m = _model(fx).eval()
    beam = D.BeamCTCDecoder(fx.labels, beam_width=10)
    tgt = D.GreedyDecoder(fx.labels)
    m.attach_evaluation(beam, D.WordErrorRate(decoder=beam, target_decoder=tgt), D.CharErrorRate(decoder=beam, target_decoder=tgt))
    seen = {}
    fwd = m.forward

    def forward(*a, **k):
        seen["out"] = fwd(*a, **k)
        return seen["out"]
    m.forward = forward
    logged = {}
    m.log = lambda k, v, **kw: logged.__setitem__(k, v)
    inputs, targets, pct, tsz = fx.batch()
    with torch.no_grad():
        m.validation_step((torch.from_numpy(inputs), torch.from_numpy(targets), torch.from_numpy(pct.copy()), torch.from_numpy(tsz)), 0)
    out, out_sizes, _ = seen["out"]
    strings, _ = beam.decode(out, out_sizes)
    hyp = [s[0] for s in strings]
    refs, o = [], 0
    for s in tsz:
        refs.append(''.join(fx.labels[int(v)] for v in targets[o:o + int(s)]))
        o += int(s)
    werr = wtot = cerr = ctot = 0
    for h, r in zip(hyp, refs):
        vocab = {w: chr(i) for i, w in enumerate(set(h.split() + r.split()))}
        werr += _edit(''.join(vocab[w] for w in h.split()), ''.join(vocab[w] for w in r.split()))
        wtot += len(r.split())
        cerr += _edit(h.replace(' ', ''), r.replace(' ', ''))
        ctot += len(r.replace(' ', ''))
    assert set(logged) == {"wer", "cer"}
    assert abs(float(logged["wer"]) - float(werr) / wtot * 100) <= 1e-9
    assert abs(float(logged["cer"]) - float(cerr) / ctot * 100) <= 1e-9
    assert any(hyp)


def test_decode_host_tensor_without_sizes():
    """The reference's run_transcribe passes out.cpu() and no sizes (inference.py:96-98); fp64 input is converted."""
    from deepspeech.pytorch_amd.configs import LABELS
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    p = _probs(np.random.default_rng(11), 2, 50, len(LABELS))
    dec = BeamCTCDecoder(LABELS, beam_width=8)
    strings, offsets = dec.decode(torch.from_numpy(p).double())
    assert len(strings) == 2 and all(len(s) == 8 for s in strings) and all(len(o) == 8 for o in offsets)
    for n in range(2):
        ref = beam_search(p[n], 50, 0, 8, 40, 1.0)["beams"]
        assert strings[n][0] == ''.join(LABELS[c] for c in ref[0][0])
        assert offsets[n][0].dtype == torch.int32 and tuple(offsets[n][0].tolist()) == ref[0][1]
    s2, _, sc = dec.decode_beams(torch.from_numpy(p).to(DEV), torch.tensor([50, 50]))
    assert s2 == strings and sc.shape == (2, 8) and bool((sc[:, 1:] >= sc[:, :-1]).all())
