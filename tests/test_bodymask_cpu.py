"""The host body-mask utility (ganslate_amd/data/utils/body_mask.py) and `pad` (data/utils/ops.py): get_body_mask against
the plain-numpy restatement of the definition in tests/bodymask_ref.py on every case of that module, both against
scipy.ndimage.label + binary_fill_holes where scipy imports, apply_body_mask and pad against their reference expressions.
Everything is integer or boolean: equality is exact."""
import numpy as np
import pytest

from tests import bodymask_ref as R

CASES = R.cases()
NON_EMPTY = [n for n in CASES if n != "none_inside"]


@pytest.mark.parametrize("name", NON_EMPTY)
def test_host_body_mask_equals_the_definition(name):
    from ganslate_amd.data.utils.body_mask import get_body_mask
    v, t = CASES[name]
    want, (count, first) = R.expected(name)
    got = get_body_mask(v, t)
    assert got.dtype == np.uint8 and got.shape == v.shape
    assert np.array_equal(got, want)
    assert count > 0 and want.ravel()[first] == 1
    if v.dtype == np.int16:                                   # the same volume as fp32 gives the same mask
        assert np.array_equal(get_body_mask(v.astype(np.float32), t), want)


@pytest.mark.parametrize("name", NON_EMPTY)
def test_definition_equals_scipy(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    v, t = CASES[name]
    with np.errstate(invalid="ignore"):
        b = v.astype(np.float32) >= np.float32(t)
    lab, n = ndimage.label(b)
    counts = [int(np.sum(lab == k)) for k in range(1, n + 1)]
    comp = lab == int(np.argmax(counts)) + 1
    want = np.stack([ndimage.binary_fill_holes(s) for s in comp]).astype(np.uint8)
    got, (count, first) = R.expected(name)
    assert np.array_equal(got, want)
    assert count == max(counts) and first == int(np.flatnonzero(comp.ravel())[0])


def test_the_cases_hold_what_they_are_named_for():
    mask, (count, first) = R.expected("tie")
    assert count == 18 and first == 1 * 100 + 1 * 10 + 1 and mask.sum() == 18 and mask[1, 6, 5] == 0
    mask, _ = R.expected("hollow_box")
    assert mask[3, 5, 5] == 1 and mask[1, 5, 5] == 1 and mask[4, 5, 5] == 0 and mask[4, 5, 2] == 0
    mask, _ = R.expected("diagonal_ring")
    assert mask[0, 2, 2] == 1 and mask[0, 4, 4] == 1 and mask[0, 1, 1] == 0
    mask, (count, _) = R.expected("all_inside")
    assert mask.all() and count == mask.size
    mask, (count, first) = R.expected("equal_to_threshold")
    assert (count, first) == (1, 1 * 30 + 2 * 6 + 3) and mask.sum() == 1
    mask, info = R.expected("none_inside")
    assert not mask.any() and info == (0, -1)
    serp = R.serpentine()
    mask, (count, first) = R.expected("serpentine")
    path = serp[:, :, :30]
    assert first == 0 and count == int(path.sum()) == int(serp[:, :, 32:].sum()) + 1      # one component, decoy one smaller
    assert np.array_equal(mask[:, :, :30] != 0, path) and not mask[:, :, 30:].any()
    for name in ("random_12x20x24_0.62", "random_12x20x24_0.8", "random_5x9x11_0.8"):
        v, t = CASES[name]
        _, (_, first) = R.expected(name)
        assert first != int(np.flatnonzero((v >= t).ravel())[0]), name                      # the largest is not the first


def test_no_voxel_at_the_threshold_raises():
    from ganslate_amd.data.utils.body_mask import apply_body_mask, get_body_mask
    v, t = CASES["none_inside"]
    with pytest.raises(ValueError, match="no voxel reaches the threshold"):
        get_body_mask(v, t)
    with pytest.raises(ValueError):
        apply_body_mask(v, hu_threshold=t)
    with pytest.raises(ValueError, match="D, H, W"):
        get_body_mask(np.zeros((4, 4)), 0)


def test_apply_body_mask():
    from ganslate_amd.data.utils.body_mask import apply_body_mask
    v, _ = CASES["hollow_box"]
    mask, _ = R.expected("hollow_box")
    got = apply_body_mask(v)                                   # defaults: value -1024 outside, threshold -300
    assert np.array_equal(got, np.where(mask, v, -1024))
    assert np.array_equal(apply_body_mask(v, masking_value=7, hu_threshold=-300), np.where(mask, v, 7))
    assert apply_body_mask(v, apply_mask=False) is v


@pytest.mark.parametrize("shape,target", [((5, 9, 11), (8, 9, 16)), ((5, 9, 11), (6, 12, 12)), ((5, 9, 11), (4, 9, 30)),
                                          ((12, 20, 24), (12, 20, 24)), ((3, 4, 5), (2, 3, 4))])
def test_pad(shape, target):
    from ganslate_amd.data.utils.ops import pad
    rng = np.random.default_rng(3)
    v = rng.integers(-50, 50, size=shape).astype(np.int16)
    widths = []
    for s, t in zip(shape, target):
        total = t - s if t > s else 0
        widths.append((total // 2, total // 2 + total % 2))
    want = np.pad(v, widths, "constant", constant_values=v.min())
    got = pad(v, target)
    assert got.shape == tuple(max(s, t) for s, t in zip(shape, target)) and got.dtype == v.dtype
    assert np.array_equal(got, want)
    inner = tuple(slice(w[0], w[0] + s) for w, s in zip(widths, shape))
    assert np.array_equal(got[inner], v)
    outer = np.ones(got.shape, bool)
    outer[inner] = False
    assert (got[outer] == v.min()).all()
    ones = np.ones(shape, np.uint8)
    assert pad(ones, target).all()                             # an all-ones mask pads with 1
    with pytest.raises(ValueError):
        pad(v, target[:2])
    assert np.array_equal(R.volume_prepare([v], ones, [], target, [0.0], [1.0], [-50.0], [50.0])[1][0], pad(ones, target))
    assert R.pad_widths(shape, target) == widths


def test_nothing_under_the_package_imports_scipy():
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent / "ganslate_amd"
    hits = [str(p) for p in root.rglob("*.py") if "import scipy" in p.read_text() or "from scipy" in p.read_text()]
    assert not hits
