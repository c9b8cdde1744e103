"""The image-op spec (preprocess/ops_ref.py) pinned at the shapes of ``image_shapes.SHAPES``:
against SciPy where SciPy has the op, against plain loops written from the definition where
it does not (NL-means, even erode / dilate windows), and the reflection rule itself."""
import numpy as np
import pytest
import scipy.ndimage as ndi

import image_shapes as S
from cloud_server_amd.preprocess import ops_ref


def _ids(shapes):
    return [f"{h}x{w}" for h, w in shapes]


shape_param = pytest.mark.parametrize("hw", S.GENERAL_SHAPES, ids=_ids(S.GENERAL_SHAPES))


def test_shape_table_is_complete():
    assert set(S.LIMIT_SHAPES) <= set(S.SHAPES) and len(S.GENERAL_SHAPES) == len(S.SHAPES) - 3
    assert all(isinstance(why, str) and why for why in S.SHAPES.values())


def test_nlmeans_select_matches_the_launcher_table():
    """The kernel each shape takes, worked out once from csa_img_nlmeans' conditions: an edit
    to the thresholds must not move every case onto one kernel unnoticed."""
    table = {(28, 28): "box", (20, 36): "box", (36, 20): "box", (32, 32): "box", (7, 100): "box",
             (33, 32): "direct", (40, 33): "direct", (64, 48): "direct", (102, 102): "direct",
             (103, 102): "refused", (102, 103): "refused"}
    for hw, want in table.items():
        assert S.nlmeans_select(*hw) == want, hw


def test_generators():
    a = S.smooth_u8(3, 20, 36)
    assert a.shape == (3, 20, 36) and a.dtype == np.uint8 and len(np.unique(a)) > 50
    assert np.array_equal(a, S.smooth_u8(3, 20, 36)) and not np.array_equal(a[0], a[1])
    r = S.random_u8(5, 9, 8, seed=2)
    assert r.shape == (5, 9, 8) and r.dtype == np.uint8 and len({x.tobytes() for x in r}) == 5


# ---------------------------------------------------------------- linear filters vs SciPy
@shape_param
def test_mean_filter_matches_scipy(hw):
    x = S.random_u8(3, *hw, seed=4)
    for k in (1, 3, 4, 5, 8):
        ref = ndi.uniform_filter(x.astype(np.float64), size=(1, k, k), mode="mirror")
        d = np.abs(ops_ref.mean_filter(x, k).astype(np.int64) - np.rint(ref)).max()
        assert d <= 1, (k, d)


@shape_param
def test_gaussian_matches_scipy(hw):
    x = S.random_u8(3, *hw, seed=5)
    for k in (1, 3, 9):
        g = ops_ref.gaussian_kernel(k)
        ref = ndi.correlate(x.astype(np.float64), np.outer(g, g)[None], mode="mirror")
        d = np.abs(ops_ref.gaussian_blur(x, k).astype(np.int64) - np.rint(ref)).max()
        assert d <= 1, (k, d)


# ---------------------------------------------------------------- rank filters
@shape_param
def test_median_erode_dilate_match_scipy(hw):
    x = S.random_u8(3, *hw, seed=6)
    for k in (3, 7):
        assert np.array_equal(ops_ref.median_filter(x, k), ndi.median_filter(x, size=(1, k, k), mode="nearest")), k
    for k in (3, 4, 6):
        assert np.array_equal(ops_ref.erode(x, k), ndi.grey_erosion(x, size=(1, k, k), mode="nearest")), k
    for k in (3, 5):
        assert np.array_equal(ops_ref.dilate(x, k), ndi.grey_dilation(x, size=(1, k, k), mode="nearest")), k


@shape_param
def test_even_windows_follow_the_anchor(hw):
    """SciPy's grey_dilation reflects an even window, so it is no reference for dilate at even
    k: the definition (cv2's anchor k // 2, taps outside the image ignored) is."""
    x = S.random_u8(2, *hw, seed=7)
    for k in (4, 6):
        for i in range(len(x)):
            assert np.array_equal(ops_ref.dilate(x, k)[i], S.window_loop(x[i], k, max)), (k, i)
            assert np.array_equal(ops_ref.erode(x, k)[i], S.window_loop(x[i], k, min)), (k, i)


# ---------------------------------------------------------------- NL-means vs the definition
@pytest.mark.parametrize("h", [15, 4])
def test_nlmeans_matches_the_loop(h):
    x = S.smooth_u8(1, 7, 11, seed=3)
    assert np.array_equal(ops_ref.nl_denoise_gray(x, h)[0], S.nlmeans_loop(x[0], float(h)))


# ---------------------------------------------------------------- reflection
@pytest.mark.parametrize("n,r", [(3, 4), (2, 15), (5, 15), (1, 3)])
def test_numpy_reflect_is_the_kernels_reflect101(n, r):
    """Radii beyond n - 1 bounce more than once: the device loop is a ``while``."""
    a = np.arange(10, 10 + n)
    want = np.array([a[S.reflect101(i, n)] for i in range(-r, n + r)])
    assert np.array_equal(np.pad(a, r, mode="reflect"), want)
    img = np.arange(n * 2).reshape(n, 2)
    assert np.array_equal(ops_ref._pad_reflect101(img[None], r)[0], S.pad_reflect101(img, r))
