"""Host checks (-m "not gpu") of the beam-search restatement the GPU tests rely on (tests/beam_reference.py): with a beam wide
enough to hold every prefix and no pruning it is exact (brute force over all C^T paths, torch's CTC loss); with a narrow beam it
only loses paths.  Plus the decoder class's refusal of a language model, which needs no device."""
import numpy as np
import pytest
import torch

from beam_reference import FLT_MIN, beam_search, brute_force, prune


def _probs(rng, T, C, scale=2.0):
    z = rng.standard_normal((T, C)) * scale
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


TINY = [(1, 2), (2, 3), (3, 3), (4, 3), (5, 3), (6, 3), (4, 4), (5, 4)]


@pytest.mark.parametrize("T,C", TINY)
def test_wide_beam_equals_brute_force(T, C):
    rng = np.random.default_rng(100 * T + C)
    p = _probs(rng, T, C)
    exact = brute_force(p)
    res = beam_search(p, T, 0, beam_width=10 ** 6, cutoff_top_n=C, cutoff_prob=1.0, dtype=np.float64)
    got = {lab: s for lab, _, s in res["beams"]}
    assert set(got) == set(exact)
    for lab, s in exact.items():
        assert abs(got[lab] - s) <= 1e-9 * max(1.0, abs(s)), (lab, got[lab], s)
    scores = [s for _, _, s in res["beams"]]
    assert scores == sorted(scores)                          # rank order = best first


@pytest.mark.parametrize("T,C", TINY)
def test_wide_beam_equals_torch_ctc_loss(T, C):
    rng = np.random.default_rng(7 + 100 * T + C)
    p = _probs(rng, T, C, scale=1.0)
    res = beam_search(p, T, 0, beam_width=10 ** 6, cutoff_top_n=C, cutoff_prob=1.0, dtype=np.float64)
    lp = torch.log(torch.from_numpy(p).double() + float(FLT_MIN))[:, None, :]
    for lab, _, s in res["beams"]:
        if not lab:
            ref = -float(lp[:, 0, 0].sum())                  # the empty string: every frame blank
        else:
            tgt = torch.tensor([lab], dtype=torch.long)
            ref = float(torch.nn.functional.ctc_loss(lp, tgt, torch.tensor([T]), torch.tensor([len(lab)]), blank=0,
                                                     reduction="none", zero_infinity=False)[0])
        assert abs(s - ref) <= 1e-9 * max(1.0, abs(ref)), (lab, s, ref)


@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_narrow_beam_only_loses_paths(B):
    rng = np.random.default_rng(B)
    for _ in range(5):
        p = _probs(rng, 6, 4)
        exact = brute_force(p)
        res = beam_search(p, 6, 0, beam_width=B, cutoff_top_n=4, cutoff_prob=1.0, dtype=np.float64)
        assert 1 <= len(res["beams"]) <= B
        labs = [lab for lab, _, _ in res["beams"]]
        assert len(set(labs)) == len(labs)                   # no string twice
        for lab, _, s in res["beams"]:
            assert s >= exact[lab] - 1e-9 * max(1.0, abs(exact[lab]))


def test_offsets_and_greedy_path():
    # B = 1, top-1 pruning: the greedy path (arg-max per frame, repeats collapsed, blanks removed), each label at the first
    # frame of its run
    rng = np.random.default_rng(3)
    p = _probs(rng, 40, 5, scale=3.0)
    res = beam_search(p, 40, 0, beam_width=1, cutoff_top_n=1, cutoff_prob=1.0)
    a = p.argmax(axis=1)
    labs, frames = [], []
    for t, c in enumerate(a):
        if c != 0 and (t == 0 or c != a[t - 1]):
            labs.append(int(c))
            frames.append(t)
    (lab, fr, _), = res["beams"]
    assert lab == tuple(labs) and fr == tuple(frames)


def test_prune_rules():
    p = np.array([[0.1, 0.4, 0.4, 0.05, 0.05]], np.float32)
    (kc, kp), = prune(p, 3, 1.0)
    assert kc.tolist() == [1, 2, 0]                          # descending, lower class first on the tie
    (kc, kp), = prune(p, 40, 0.85)
    assert kc.tolist() == [1, 2, 0]                          # 0.4 + 0.4 < 0.85 <= 0.9
    (kc, kp), = prune(p, 2, 0.85)
    assert kc.tolist() == [1, 2]                             # cutoff_top_n caps the cumulative cut
    (kc, kp), = prune(p, 40, 1.0)
    assert kc.tolist() == [0, 1, 2, 3, 4]                    # no pruning


def test_empty_utterance():
    res = beam_search(np.full((3, 4), 0.25, np.float32), 0, 0, beam_width=4)
    assert res["beams"] == [((), (), 0.0)]


def test_beam_decoder_refuses_a_language_model():
    from deepspeech.pytorch_amd.configs import LABELS
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    with pytest.raises(ValueError, match="not implemented"):
        BeamCTCDecoder(LABELS, lm_path="x.arpa")
    dec = BeamCTCDecoder(LABELS, alpha=0.5, beta=1.0, num_processes=8)     # alpha / beta without an LM are ignored
    assert dec.beam_width == 100 and dec.cutoff_top_n == 40 and dec.cutoff_prob == 1.0 and dec.blank_index == 0
