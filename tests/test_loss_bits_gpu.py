"""csrc/loss.hip bit for bit against tests/golden/loss_bits.json, which tools/gen_golden_loss_bits.py recorded on the MI355X from
the library of the commit named in the file (cases, inputs and the reason for every shape: tests/loss_bits_cases.py). Equality
only: a pattern or digest that differs names its case."""
import json
from pathlib import Path

import pytest

from tests import loss_bits_cases as B

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((Path(__file__).parent / "golden" / "loss_bits.json").read_text())["results"]
_RUN = {}


def run_group(ops, group):
    if group not in _RUN:
        _RUN[group] = B.run_group(ops, group)
    return _RUN[group]


@pytest.mark.parametrize("group", B.GROUPS)
def test_loss_bits_are_those_of_the_recorded_library(hip_ops, group):
    got = run_group(hip_ops, group)
    want = {k: v for k, v in GOLDEN.items() if k.startswith(group + "/")}
    assert sorted(got) == sorted(want), "the cases run and the cases recorded differ"
    wrong = [f"{k}: got {got[k]} recorded {want[k]}" for k in sorted(got) if got[k] != want[k]]
    print(f"{group}: {len(got)} patterns and digests compared")
    assert not wrong, "\n".join(wrong)


def test_identical_images_give_zero_and_no_gradient(hip_ops):
    """y == x: S is exactly 0 at every pixel (ssim_terms / ssim_s_double without contraction), so the value's bits are 0 and
    every gradient element is 0.0 — from the formula, independent of the recorded file"""
    got = {k: v for k, v in run_group(hip_ops, "ssim").items() if "identical" in k}
    H, W = B.SSIM_PLANES[-1]
    shapes = {"ssim/dense_identical": (1, 3, H, W), "ssim/window_identical_1-3": (2, 2, H, W)}
    assert len(got) == 5 + 3
    for k, v in got.items():
        want = B.ZERO_BITS if k.endswith("/value") else B.zeros_digest(shapes[k.split("/" + f"{H}x{W}")[0]])
        assert v == want, k
