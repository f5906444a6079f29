"""dvs_image_metrics_views (csrc/metrics.hip) on the GPU against the numpy fp64 restatement of tests/metrics_ref.py, on the smallest
shapes at which the kernel can go wrong: not a multiple of the 16x16 tile and several tiles (37x53), smaller than the halo and than
one tile (7x9), exactly one tile (16x16), 8-bit targets on an odd byte stride (33x130), the full 16 views of one launch (20x20).

Bars:
  ssim  |d| < 2e-5        the bar tests/test_gpu_train_ops.py::test_ssim_forward_backward holds dvs_ssim_forward to (same arithmetic)
  mse, l1  relative 1e-5  one missing or doubled pixel at 37x53 moves them by 1/(3*37*53) = 1.7e-4; fp32 terms summed as a tree in the
                          workgroup and in fp64 across workgroups err by <~ 1e-6: a decade on each side
  psnr  |d| < 1e-4 dB     4.34 * d(mse)/mse at the bar above, rounded up
"""
import ctypes as C
import numpy as np
import pytest
from metrics_ref import image_metrics_np, assert_metrics_close
from train_step_ref import pack_unpack_u8, ellipse_mask

pytestmark = pytest.mark.gpu


def _views(seed, V, H, W, u8=False):
    """rendered views in [-0.2, 1.3] (the clamp matters) near their targets; targets fp32 in [0, 1], or 8-bit with their fp32 expansion"""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(0, 1, (V, 3, H, W)).astype(np.float32)
    img = np.clip(tgt + 0.3 * rng.standard_normal((V, 3, H, W)), -0.2, 1.3).astype(np.float32)
    if not u8:
        return img, tgt, tgt
    bytes_ = np.rint(np.clip(tgt * np.float32(255.0), 0, 255)).astype(np.uint8)
    return img, bytes_, pack_unpack_u8(tgt)


def _run(dev, img, tgt, masks=None):
    import torch
    from divshot_amd.train_ops import image_metrics
    t = lambda a: None if a is None else torch.tensor(a, device=dev)
    out = image_metrics([t(a) for a in img], [t(a) for a in tgt], None if masks is None else [t(a) for a in masks])
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(img), 4)
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def three_views(gpu_device):
    H, W = 37, 53
    img, tgt, ref_t = _views(1, 3, H, W)
    masks = [None, ellipse_mask(W, H), None]
    return img, tgt, masks, _run(gpu_device, img, tgt, masks)


def test_three_views_fp32_targets_mask_on_one(three_views):
    img, tgt, masks, out = three_views
    assert (img < 0).any() and (img > 1).any() and 0 < masks[1].mean() < 1
    for v in range(3):
        assert_metrics_close(out[v], image_metrics_np(img[v], tgt[v], masks[v]), f"37x53 view {v}")
    # the mask and the clamp are in the numbers: without them the restatement is far outside the bars
    assert abs(image_metrics_np(img[1], tgt[1], None)[0] - out[1][0]) > 1e-3 * out[1][0]
    assert abs(float(((img[0].astype(np.float64) - tgt[0]) ** 2).mean()) - out[0][0]) > 1e-3 * out[0][0]


@pytest.mark.parametrize("H,W,V,u8", [(7, 9, 1, False), (16, 16, 1, False), (33, 130, 2, True), (20, 20, 16, False)])
def test_shapes(gpu_device, H, W, V, u8):
    img, tgt, ref_t = _views(10 + H, V, H, W, u8)
    out = _run(gpu_device, img, tgt)
    for v in range(V):
        assert_metrics_close(out[v], image_metrics_np(img[v], ref_t[v]), f"{H}x{W} view {v}{' u8' if u8 else ''}")


def test_identical_images(gpu_device):
    _, tgt, _ = _views(3, 2, 37, 53)
    out = _run(gpu_device, tgt, tgt, [ellipse_mask(53, 37), None])
    for v in range(2):
        assert out[v][0] == 0.0 and out[v][1] == 0.0 and out[v][3] == 100.0 and abs(out[v][2] - 1.0) < 1e-5, out[v]


def test_reproducible_and_independent_of_the_batch(gpu_device, three_views):
    img, tgt, masks, out = three_views
    again = _run(gpu_device, img, tgt, masks)
    assert out.tobytes() == again.tobytes()                 # bit for bit, not merely close
    for v in range(3):
        alone = _run(gpu_device, img[v:v + 1], tgt[v:v + 1], masks[v:v + 1])
        assert alone[0].tobytes() == out[v].tobytes(), (v, alone[0], out[v])


def test_argument_checks(gpu_device):
    import torch
    from divshot_amd._lib import lib, MetricsView
    H = W = 16
    x = torch.zeros((3, H, W), device=gpu_device)
    scratch = torch.empty(lib.dvs_image_metrics_scratch_bytes(W, H, 16), dtype=torch.uint8, device=gpu_device)
    out = torch.empty((17, 4), dtype=torch.float64, device=gpu_device)
    arr = (MetricsView * 17)()
    for a in arr:
        a.img, a.target, a.mask = x.data_ptr(), x.data_ptr(), None
    call = lambda n, s=scratch.data_ptr(), o=out.data_ptr(): lib.dvs_image_metrics_views(None, arr, n, W, H, 0, C.c_void_p(s), C.c_void_p(o))
    INVALID = 1                                              # DVS_ERR_INVALID
    assert call(0) == INVALID and call(17) == INVALID and call(-1) == INVALID
    assert call(1) == 0 and call(16) == 0
    arr[1].img = None
    assert call(2) == INVALID and call(1) == 0               # a NULL img among the views that are used
    arr[1].img, arr[0].target = x.data_ptr(), None
    assert call(1) == INVALID
    arr[0].target = x.data_ptr()
    assert call(1, s=None) == INVALID and call(1, o=None) == INVALID
    assert lib.dvs_image_metrics_views(None, arr, 1, 0, H, 0, scratch.data_ptr(), out.data_ptr()) == INVALID
    assert lib.dvs_image_metrics_views(None, arr, 1, W, -3, 0, scratch.data_ptr(), out.data_ptr()) == INVALID
    torch.cuda.synchronize()
