"""HIP image-op kernels vs the NumPy spec at the shapes of ``image_shapes.SHAPES`` (GPU only):
non-square images, both NL-means kernels, the grid-stride trips of the elementwise kernels,
the sizes that need the opt-in LDS, and every launcher refusal.

Exact ops are compared with ``np.array_equal``.  NL-means and resize keep the criterion of
``test_gpu_image_ops`` (max |d| <= 1, share of differing pixels < 1e-3) over at least 10,000
output pixels a case, so the share has a resolution of ten pixels.  Measured figures:
profiles/image_ops_parity.md."""
import json
import os
import shutil
import zipfile

import numpy as np
import pytest
import torch

import image_shapes as S
from cloud_server_amd.ops import fused as K
from cloud_server_amd.preprocess import gpu, ops_ref, pipeline

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(__file__), "fixtures")
N = 5
SENTINEL = 0xA5


def _id(hw):
    return f"{hw[0]}x{hw[1]}"


def _shapes(ok=lambda h, w: True):
    return pytest.mark.parametrize("hw", [s for s in S.GENERAL_SHAPES if ok(*s)], ids=_id)


def _exact(name, x, v1=None, v2=None, mode="saturate", seed=None):
    def rng():                                       # both sides draw the same counter-RNG seed from it
        return None if seed is None else np.random.default_rng(seed)
    ref = ops_ref.apply_op(name, x, v1, v2, mode=mode, rng=rng())
    got = gpu.apply_op(name, x, v1, v2, mode=mode, rng=rng())
    assert got.dtype == np.uint8 and got.shape == ref.shape
    bad = got != ref
    assert not bad.any(), (name, v1, v2, x.shape[1:], int(np.abs(got.astype(int) - ref).max()), float(bad.mean()),
                           np.argwhere(bad)[:4].tolist())


def _close(got, ref, what):
    d = np.abs(got.astype(int) - ref.astype(int))
    print(f"{what}: pixels {d.size} max {int(d.max())} differing {int((d > 0).sum())} share {(d > 0).mean():.2e}")
    assert d.size >= 10000
    assert d.max() <= 1 and (d > 0).mean() < 1e-3, what


# ----------------------------------------------------------------------- exact ops
@_shapes()
def test_flips(hw):
    x = S.random_u8(N, *hw, seed=10)
    for name in ("flip_up_down", "flip_left_right", "transpose_image"):
        _exact(name, x)


@_shapes()
def test_affine(hw):
    x = S.random_u8(N, *hw, seed=11)
    x[0, 0, 0], x[1, -1, -1] = 0, 255
    for a, b in ((1.37, -12), (-1.3, 300)):          # both clamps
        _exact("adjust_brightness_contrast", x, a, b)
    for a, b in ((1.9, 30), (-1.3, -40)):            # wrap; the truncated value is negative in the second
        _exact("adjust_brightness_contrast", x, a, b, mode="wrap")
    for mode in ("saturate", "wrap"):
        _exact("random_brightness_contrast", x, 1.8, 25, mode=mode, seed=12)


@_shapes(S.sep_ok)
def test_linear_filters(hw):
    x = S.random_u8(N, *hw, seed=13)
    for k in (1, 4, 5, 8):
        _exact("mean_filter", x, k)
    for k in (1, 9, 31):
        _exact("gaussian_blur", x, k)


@_shapes(S.rank_ok)
def test_rank_filters(hw):
    x = S.random_u8(N, *hw, seed=14)
    for k in (1, 3, 7):
        _exact("median_filter", x, k)
    for k in (1, 4, 5):
        _exact("erode", x, k)
        _exact("dilate", x, k)


def test_window_wider_than_the_image():
    """k >= 2 * max(H, W): every window holds the whole image, whatever the anchor."""
    x = S.random_u8(N, 20, 36, seed=15)
    lo = np.broadcast_to(x.min(axis=(1, 2), keepdims=True), x.shape)
    hi = np.broadcast_to(x.max(axis=(1, 2), keepdims=True), x.shape)
    for k in (72, 300, 1 << 30):
        assert np.array_equal(gpu.apply_op("erode", x, k), lo), k
        assert np.array_equal(gpu.apply_op("dilate", x, k), hi), k


@_shapes()
def test_equalize(hw):
    _exact("equalize_hist", S.random_u8(N, *hw, seed=16))


def test_equalize_constant_and_two_level():
    c = np.full((3, 20, 36), 9, np.uint8)
    c[1, :5] = 200
    c[2, :, 35] = 0
    _exact("equalize_hist", c)


@_shapes(S.clahe_ok)
def test_clahe(hw):
    _exact("clahe", S.random_u8(N, *hw, seed=17))
    _exact("clahe", S.smooth_u8(N, *hw, seed=18))


@_shapes()
def test_salt_pepper(hw):
    x = S.random_u8(N, *hw, seed=19)
    x[x == 0] = 1
    x[x == 255] = 254
    H, W = hw
    for percent in (0.07, 0.5, 1.0):                 # 0.5: m > 256 strides the draw loop at most shapes
        _exact("add_salt_pepper_noise", x, percent, seed=20)
    if H * W >= 64:                                  # at percent 1.0 the two colours collide: pepper wins
        got = gpu.apply_op("add_salt_pepper_noise", x, 1.0, rng=np.random.default_rng(20))
        assert (got == 0).sum() > (got == 255).sum() > 0


def test_limit_shapes_on_their_own_op():
    x = S.random_u8(N, 64, 128, seed=21)             # 65,536 B of dynamic LDS + 256 B static
    _exact("mean_filter", x, 5)
    _exact("gaussian_blur", x, 9)
    x = S.random_u8(N, 128, 128, seed=22)
    _exact("median_filter", x, 7)
    _exact("erode", x, 4)
    _exact("dilate", x, 5)


# ----------------------------------------------------------------------- NL-means
NLM = [((20, 36), "box"), ((36, 20), "box"), ((32, 32), "box"), ((7, 100), "box"),
       ((33, 32), "direct"), ((40, 33), "direct"), ((64, 48), "direct"), ((102, 102), "direct")]


@pytest.mark.parametrize("h", [15, 4])
@pytest.mark.parametrize("hw,kernel", NLM, ids=[f"{k}-{_id(s)}" for s, k in NLM])
def test_nlmeans(hw, kernel, h):
    assert S.nlmeans_select(*hw) == kernel
    n = max(2, -(-10000 // (hw[0] * hw[1])))
    x = S.smooth_u8(n, *hw, seed=23)
    _close(gpu.apply_op("nl_denoise_gray", x, h), ops_ref.nl_denoise_gray(x, h), f"nlmeans {kernel} {_id(hw)} h={h}")


# ----------------------------------------------------------------------- resize to 28
RESIZE = [(5, 7), (20, 36), (36, 20), (300, 400), (480, 640), (28, 685), (28, 686), (768, 1024)]


@pytest.mark.parametrize("hw", RESIZE, ids=_id)
def test_resize(hw):
    assert gpu.resize_on_device(hw[1]) == (hw[1] <= 685)
    x = S.random_u8(14, *hw, seed=24)
    x[13] = 131                                       # 13 random images (10,192 pixels) and a constant one
    ref = ops_ref.resize(x, 28)
    got = gpu.resize(x, 28)
    assert got.dtype == np.uint8 and got.shape == (14, 28, 28)
    assert np.array_equal(got[13], np.full((28, 28), 131, np.uint8))
    _close(got[:13], ref[:13], f"resize {_id(hw)}")


def test_resize_wide_device_tensor():
    x = S.random_u8(2, 28, 686, seed=25)
    got = gpu.resize(torch.from_numpy(x).cuda(), 28)
    assert got.is_cuda and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), ops_ref.resize(x, 28))


def test_pipeline_wide_images_gpu_equals_cpu(tmp_path):
    """One 768 x 1024 and one 28 x 686 upload among the dataset's images: wider than the
    device resize takes, and the GPU backend must still equal the CPU backend file for file."""
    from PIL import Image
    ops = [{"operationName": "上下翻转", "overlap": True},
           {"operationName": "高斯模糊", "value1": 5, "overlap": False}]
    wide = {"wide_photo.png": S.smooth_u8(1, 768, 1024, seed=26)[0], "wide_strip.png": S.random_u8(1, 28, 686, seed=27)[0]}
    res = {}
    for be in ("cpu", "gpu"):
        d = tmp_path / be
        with zipfile.ZipFile(os.path.join(FIX, "test-pics.zip")) as z:
            z.extractall(d / "data")
        with open(os.path.join(FIX, "tag.json"), encoding="utf-8") as f:
            tags = json.load(f)
        for name, img in wide.items():
            Image.fromarray(img, mode="L").save(d / "data" / name)
            tags[name] = "7"
        with open(d / "tag.json", "w", encoding="utf-8") as f:
            json.dump(tags, f)
        out = pipeline.run(str(d / "data"), str(d / "tag.json"), ops, backend=be, seed=5)
        res[be] = (out, {n: pipeline._read(str(d / "data" / n)) for n in out})
    assert res["cpu"][0] == res["gpu"][0] and len(res["cpu"][0]) == (99 + 2) * 2
    for n, a in res["cpu"][1].items():
        assert a.shape == (28, 28) and np.array_equal(a, res["gpu"][1][n]), n


# ----------------------------------------------------------------------- grid-stride trips
NBIG = 21500                                          # 21,500 * 784 = 16,856,000 > 16,777,216


@pytest.fixture(scope="module")
def big():
    assert NBIG * 784 > S.ELEMENTWISE_CAP > (NBIG - 101) * 784
    return S.random_u8(NBIG, 28, 28, seed=28)


def _tail_equal(got, ref):
    """Equality of the whole batch, reported apart for the images the loop's second trip wrote."""
    first = S.ELEMENTWISE_CAP // 784                  # the first image the second trip touches
    assert np.array_equal(got[first:], ref[first:]), "second trip"
    assert np.array_equal(got[:first], ref[:first]), "first trip"


def test_grid_stride_flip_and_affine(big):
    _tail_equal(gpu.apply_op("flip_left_right", big), ops_ref.flip_left_right(big))
    _tail_equal(gpu.apply_op("adjust_brightness_contrast", big, 1.37, -12),
                ops_ref.adjust_brightness_contrast(big, 1.37, -12))
    # per-image parameters: the second trip's n = i / HW picks the draws of the last images
    _tail_equal(gpu.apply_op("random_brightness_contrast", big, 1.8, 25, rng=np.random.default_rng(29)),
                ops_ref.random_brightness_contrast(big, 1.8, 25, rng=np.random.default_rng(29)))


def test_grid_stride_infer_prep():
    x = S.random_u8(NBIG, 20, 20, seed=30)
    canvas = np.zeros((NBIG, 28, 28), np.uint8)
    canvas[:, 4:24, 4:24] = np.where(x > 150, 254, 0)
    got = gpu.infer_prep(x).cpu().numpy()
    _tail_equal(got, (canvas.astype(np.float32) / 255.0).reshape(NBIG, 784).astype(np.float32))
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.full((NBIG, 784), SENTINEL, dtype=torch.uint8, device="cuda")
    assert gpu._lib().csa_img_infer_prep_u8(K.ptr(d_in), K.ptr(d_out), NBIG, K.stream()) == 0
    _tail_equal(d_out.cpu().numpy(), canvas.reshape(NBIG, 784))


# ----------------------------------------------------------------------- refusals
def test_launchers_refuse_without_launching():
    """Every limit of every launcher: a non-zero return and an untouched output buffer.  The
    buffers are larger than any refused shape, N is 1 where it is not the thing refused."""
    lib = gpu._lib()
    st = K.stream()
    size = 1 << 16
    x = torch.zeros(size, dtype=torch.uint8, device="cuda")
    out = torch.full((size,), SENTINEL, dtype=torch.uint8, device="cuda")
    fout = torch.full((size,), -123.0, device="cuda")
    dbl = torch.full((64,), 1.0 / 32, dtype=torch.float64, device="cuda")
    iy, wy = ops_ref._resize_axis_weights(28, 28)
    ix, wx = ops_ref._resize_axis_weights(686, 28)
    tabs = [gpu._d(iy, torch.int32), gpu._d(wy, torch.float64), gpu._d(ix, torch.int32), gpu._d(wx, torch.float64)]
    tp = [K.ptr(t) for t in tabs]
    xp, op, dp = K.ptr(x), K.ptr(out), K.ptr(dbl)

    # name -> call(in, out, N, H, W) with otherwise valid arguments
    calls = {
        "flip": lambda i, o, n, h, w: lib.csa_img_flip(i, o, n, h, w, 1, st),
        "affine": lambda i, o, n, h, w: lib.csa_img_affine(i, o, n, h, w, dp, dp, 0, st),
        "affine_rand": lambda i, o, n, h, w: lib.csa_img_affine_rand(i, o, n, h, w, 7, 1.5, 20, 0, st),
        "salt_pepper_rand": lambda i, o, n, h, w: lib.csa_img_salt_pepper_rand(i, o, n, h, w, 7, 10, st),
        "sep_filter": lambda i, o, n, h, w: lib.csa_img_sep_filter(i, o, n, h, w, dp, 3, st),
        "median": lambda i, o, n, h, w: lib.csa_img_rank_filter(i, o, n, h, w, 3, 0, st),
        "erode": lambda i, o, n, h, w: lib.csa_img_rank_filter(i, o, n, h, w, 3, 1, st),
        "equalize": lambda i, o, n, h, w: lib.csa_img_equalize(i, o, n, h, w, st),
        "clahe": lambda i, o, n, h, w: lib.csa_img_clahe(i, o, n, h, w, 8, 40.0, st),
        "nlmeans": lambda i, o, n, h, w: lib.csa_img_nlmeans(i, o, n, h, w, 10.0, 7, 21, st),
        "resize": lambda i, o, n, h, w: lib.csa_img_resize(i, o, n, h, w, 28, *tp, st),
    }
    for name, call in calls.items():
        for n, h, w in ((0, 28, 28), (-1, 28, 28), (1, 0, 28), (1, 28, 0), (1, -28, 28), (1, 28, -28),
                        (1, 1 << 16, 1 << 16)):      # H * W = 2^32 wraps to 0 as an int product
            assert call(xp, op, n, h, w) != 0, (name, n, h, w)
    for name in ("flip", "salt_pepper_rand", "sep_filter", "median", "erode", "clahe", "nlmeans", "resize"):
        assert calls[name](xp, xp, 1, 28, 28) != 0, name            # in == out
    assert lib.csa_img_infer_prep(xp, K.ptr(fout), 0, st) != 0
    assert lib.csa_img_infer_prep_u8(xp, op, 0, st) != 0

    assert lib.csa_img_flip(xp, op, 1, 28, 28, 3, st) != 0
    assert lib.csa_img_affine_rand(xp, op, 1, 28, 28, 7, 1.5, -1, 0, st) != 0
    assert lib.csa_img_salt_pepper_rand(xp, op, 1, 28, 28, 7, -1, st) != 0
    assert calls["sep_filter"](xp, op, 1, 65, 127) != 0               # 8,255 > 8,192 pixels
    for k in (0, 32, -3):
        assert lib.csa_img_sep_filter(xp, op, 1, 28, 28, dp, k, st) != 0, k
    for o in ("median", "erode"):
        assert calls[o](xp, op, 1, 129, 128) != 0, o                   # 16,512 > 16,384 pixels
    for k, o in ((9, 0), (4, 0), (0, 0), (0, 1), (3, 3), (3, -1)):
        assert lib.csa_img_rank_filter(xp, op, 1, 28, 28, k, o, st) != 0, (k, o)
    for h, w in ((7, 40), (40, 7), (3, 50)):
        assert calls["clahe"](xp, op, 1, h, w) != 0, (h, w)            # H or W below the 8 tiles
    for t in (0, 9):
        assert lib.csa_img_clahe(xp, op, 1, 28, 28, t, 40.0, st) != 0, t
    for h, w in ((103, 102), (102, 103)):
        assert calls["nlmeans"](xp, op, 1, h, w) != 0, (h, w)          # padded 129 x 128
        assert S.nlmeans_select(h, w) == "refused"
    for hv in (0.0, -2.0, float("nan")):
        assert lib.csa_img_nlmeans(xp, op, 1, 28, 28, hv, 7, 21, st) != 0, hv
    for ts, ss in ((-7, 21), (7, -21), (7, 1 << 20)):
        assert lib.csa_img_nlmeans(xp, op, 1, 28, 28, 10.0, ts, ss, st) != 0, (ts, ss)
    assert calls["resize"](xp, op, 1, 28, 686) != 0                   # 28 * 686 * 8 B > 150 KB
    assert lib.csa_img_resize(xp, op, 1, 28, 686, 0, *tp, st) != 0

    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((fout == -123.0).all()) and bool((x == 0).all())
    # the neighbours of the refused shapes are accepted: the refusals above are the limits
    assert calls["sep_filter"](xp, op, 1, 64, 128) == 0 and calls["erode"](xp, op, 1, 128, 128) == 0
    assert calls["nlmeans"](xp, op, 1, 102, 102) == 0 and calls["clahe"](xp, op, 1, 8, 8) == 0
    torch.cuda.synchronize()


REFUSED = [
    ("mean_filter", (65, 127), 3), ("gaussian_blur", (65, 127), 3), ("mean_filter", (28, 28), 32),
    ("erode", (129, 128), 3), ("dilate", (129, 128), 3), ("median_filter", (129, 128), 3),
    ("clahe", (7, 40), None), ("clahe", (40, 7), None), ("clahe", (3, 50), None),
    ("nl_denoise_gray", (103, 102), 10), ("nl_denoise_gray", (28, 28), -2)]


@pytest.mark.parametrize("name,hw,v1", REFUSED, ids=[f"{n}-{_id(s)}-{v}" for n, s, v in REFUSED])
def test_apply_op_raises_on_refusal(name, hw, v1):
    with pytest.raises(RuntimeError, match="failed"):
        gpu.apply_op(name, np.zeros((1, *hw), np.uint8), v1)


def test_apply_op_median_sizes_are_value_errors():
    for k in (9, 4):
        with pytest.raises(ValueError):
            gpu.apply_op("median_filter", np.zeros((1, 28, 28), np.uint8), k)


def test_empty_batch_is_an_empty_result():
    e = np.zeros((0, 20, 36), np.uint8)
    for name in ops_ref.OP_NAMES:
        ref = ops_ref.apply_op(name, e, None, None, rng=np.random.default_rng(0))
        got = gpu.apply_op(name, e, None, None, rng=np.random.default_rng(0))
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == ref.shape == (0, 20, 36), name
    t = gpu.apply_op("clahe", torch.zeros(0, 20, 36, dtype=torch.uint8, device="cuda"))
    assert t.is_cuda and tuple(t.shape) == (0, 20, 36)
    assert gpu.resize(e, 28).shape == ops_ref.resize(e, 28).shape == (0, 28, 28)
    assert gpu.resize(np.zeros((0, 28, 686), np.uint8), 28).shape == (0, 28, 28)
    with pytest.raises(ValueError):
        gpu.apply_op("no_such_op", e)
