"""The start-offset policy of the 256x256 GEMM (csrc/ds2_gemm8.hip, ds2_gemm8_stagger_plan), asked without a device: a span only for
NT launches of at least two rounds of CUs, none for grouped TN and mixed launches, and never more than the clamp."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from deepspeech.pytorch_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_stagger_policy_rule_and_clamp(lib):
    plan = lib.ds2_gemm8_stagger_plan
    clamp = plan(-1, 0, 0)
    assert 0 < clamp <= 1000                                   # microseconds: a bad argument cannot hold a CU for long
    for cus in (1, 8, 64, 256, 304):
        for tiles in (1, cus, 2 * cus - 1):
            assert plan(0, tiles, cus) == 0                    # fewer than two rounds: no later round to keep apart
        span = plan(0, 2 * cus, cus)
        assert 0 <= span <= clamp
        for tiles in (2 * cus + 1, 2016, 100000):
            if tiles >= 2 * cus:
                assert plan(0, tiles, cus) == span             # one constant above the threshold
        for kind in (1, 2):
            for tiles in (1, 2 * cus, 2016, 100000):
                assert plan(kind, tiles, cus) == 0             # grouped TN and mixed launches keep span 0
    assert plan(0, 2016, 0) == 0                               # no CU count, no offsets
