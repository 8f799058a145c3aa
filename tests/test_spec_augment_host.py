"""Host checks of SpecAugment: the fp64 restatement (tests/spec_augment_reference.py) against the outputs of the real reference
recorded in tests/golden/specaug (tests/golden/make_spec_augment.py), and the host-side draws of augment.SpecAugment."""
import glob
import json
import os

import numpy as np
import pytest

import spec_augment_reference as R
from deepspeech.pytorch_amd.augment import SpecAugment

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "specaug")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
EPS32 = float(np.finfo(np.float32).eps)


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def noise_figures():
    """the stored max |restatement - golden| per fixture (tests/golden/specaug/README.md keeps the same table)."""
    with open(os.path.join(GOLDEN, "reference_noise.json")) as f:
        return json.load(f)


def test_fixture_set_is_complete():
    want = ["e2e_f161_t12", "e2e_f161_t63", "e2e_f161_t64", "e2e_f161_t65", "e2e_f161_t130", "e2e_f81_t40", "e2e_f5_t12",
            "hand_masks_edges", "hand_masks_width0", "hand_clamp_left", "hand_clamp_right", "hand_clamp_both_f81"]
    assert sorted(want) == FIXTURES
    assert sorted(noise_figures()) == FIXTURES


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference(name):
    """Bound = the fp32 noise of the reference itself, from its own arithmetic: it forms the query frame q = t - flow in fp32
    (rounding eps * (T + |flow|) at most; its flow carries the 1e-5 relative error of its fp32 solve that the coefficient test
    below allows, plus the residual of the affine fit) and the output moves by the largest frame-to-frame step of the clip per
    frame of q; on top come the three roundings of alpha * (hi - lo) + lo (:406-408) at the size of the values.  The figure
    reached is printed, and stored per fixture as the yardstick of the device tests."""
    z = load(name)
    x = z["x"].astype(np.float64)
    F, T = x.shape
    coef = R.warp_coef(F, T, z["pt"], int(z["i"]), int(z["d"]), z["E"])
    got = R.spec_augment(x, coef, z["fmask"], z["tmask"])
    err = float(np.abs(got - z["out"]).max())
    step = float(np.abs(np.diff(x, axis=1)).max())
    flow_err = 1e-5 * float(np.abs(z["coef_ref"]) @ np.array([F - 1, T - 1, 1.0])) + float(z["fit_resid"])
    bound = step * (EPS32 * (T + float(z["flow_absmax"])) + flow_err) + 4 * EPS32 * float(np.abs(x).max())
    print("%s: max |restatement - golden| = %.3e (bound %.3e, stored %.3e)" % (name, err, bound, noise_figures()[name]))
    assert err <= bound
    assert err <= noise_figures()[name] * 1.01 + 1e-12               # the stored yardstick is the figure of this very comparison
    # the structure the restatement rests on: no frequency flow, an affine time flow, masked cells exactly zero
    assert float(z["flow_f_absmax"]) == 0.0 and float(z["fit_resid"]) <= 1e-5
    assert np.all(z["out"][R.in_mask(F, T, z["fmask"], z["tmask"])] == 0)
    assert np.all(got[R.in_mask(F, T, z["fmask"], z["tmask"])] == 0)


@pytest.mark.parametrize("name", FIXTURES)
def test_closed_form_coefficients_match_the_reference_solve(name):
    """the fp64 closed form against the affine fit of the reference's dense flow: its fp32 4 x 4 solve (pivots of 1e-10 beside
    entries of 80) and its fp32 evaluation leave about 1e-5 of the largest flow term."""
    z = load(name)
    F, T = z["x"].shape
    coef = R.warp_coef(F, T, z["pt"], int(z["i"]), int(z["d"]), z["E"])
    scale = np.abs(coef) @ np.array([F - 1, T - 1, 1.0])
    assert np.abs(coef - z["coef_ref"]) @ np.array([F - 1, T - 1, 1.0]) <= 1e-5 * scale
    # and against the recorded solution itself: v = (a_f, a_t, a_0 - K), w
    c = np.array([F // 2, float(np.float32(z["pt"] + np.float32(z["d"]))), 1.0])
    K = float(z["w"][1]) * R.phi2(R.grid_norm(F, T) + c[0] ** 2 + c[1] ** 2)
    assert np.allclose(z["v"][:, 1] + [0, 0, K], coef, rtol=2e-5, atol=2e-5 * scale / max(F, T))
    assert np.all(z["v"][:, 0] == 0) and z["w"][0] == 0


def test_zero_coefficients_copy_the_clip():
    x = np.random.RandomState(0).standard_normal((7, 9))
    assert np.array_equal(R.warp(x, np.zeros(3)), x)
    assert not R.warp_coef(161, 10, 0.3, 5, 2, np.eye(3)).any()           # T <= 2W
    assert not R.warp_coef(161, 100, 0.3, -1, 2, np.eye(3)).any()         # i < 0


def test_draw_ranges_and_inclusive_ends():
    sa = SpecAugment(frequency_masking_para=3, time_masking_para=4, frequency_mask_num=2, time_mask_num=2, W=2)
    rng = np.random.default_rng(5)
    T, F = 7, 5
    seen_i, seen_d, seen_f, seen_t = set(), set(), set(), set()
    for _ in range(300):
        warp, fm, tm = sa.draw([T], F, rng)
        assert warp.shape == (1, 12) and warp.dtype == np.float32 and fm.shape == (1, 2, 2) and tm.shape == (1, 2, 2)
        assert fm.dtype == np.int32 and tm.dtype == np.int32 and warp[0, 11] == 0
        seen_i.add(int(warp[0, 0])), seen_d.add(int(warp[0, 1]))
        assert np.all(np.abs(warp[0, 2:11]) < 1e-9) and np.all(warp[0, 2:11] != 0)
        seen_f.update((int(s), int(w)) for s, w in fm[0]), seen_t.update((int(s), int(w)) for s, w in tm[0])
    assert seen_i == set(range(2, 5))                       # randrange(W, T - W): T - W excluded
    assert seen_d == set(range(-2, 2))                      # randrange(-W, W): W excluded
    assert seen_f == {(s, w) for w in range(3) for s in range(F - w + 1)}        # int(uniform(0, 3)) in 0..2; randint(0, F - w) inclusive
    assert seen_t == {(s, w) for w in range(4) for s in range(T - w + 1)}


def test_draw_skips_masks_wider_than_the_axis():
    sa = SpecAugment(frequency_masking_para=27, time_masking_para=70, frequency_mask_num=1, time_mask_num=1)
    rng = np.random.default_rng(1)
    for _ in range(200):
        _, fm, tm = sa.draw([12], 5, rng)
        for (s, w), size in ((fm[0, 0], 5), (tm[0, 0], 12)):
            assert (w == 0 and s == 0) or (0 <= s and s + w <= size)


def test_draw_short_clip_disables_the_warp():
    sa = SpecAugment()
    warp, _, _ = sa.draw([10, 11, 1], 161, np.random.default_rng(0))
    assert warp[0, 0] == -1 and not warp[0, 1:].any()        # T = 2W
    assert warp[1, 0] == 5                                    # T = 2W + 1: randrange(5, 6)
    assert warp[2, 0] == -1


def test_draw_is_deterministic_under_a_seed():
    sa = SpecAugment(frequency_mask_num=2, time_mask_num=3)
    a = sa.draw([100, 64, 12], 161, np.random.default_rng(42))
    b = sa.draw([100, 64, 12], 161, np.random.default_rng(42))
    c = sa.draw([100, 64, 12], 161, np.random.default_rng(43))
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    assert not all(np.array_equal(u, v) for u, v in zip(a, c))


def test_more_than_four_masks_raise():
    with pytest.raises(ValueError):
        SpecAugment(frequency_mask_num=5)
    with pytest.raises(ValueError):
        SpecAugment(time_mask_num=5)
    sa = SpecAugment()
    sa.time_mask_num = 5
    with pytest.raises(ValueError):
        sa.draw([50], 161, np.random.default_rng(0))
    SpecAugment(frequency_mask_num=4, time_mask_num=4).draw([50], 161, np.random.default_rng(0))
