"""numpy fp64 restatement of dvs_image_metrics_views (include/dvs_train.h), shared by tests/test_gpu_image_metrics.py and tests/test_eval.py.
Inputs are taken as they reach the kernel (fp32 images, fp32 or already expanded 8-bit targets, fp32 mask) and everything after that is fp64."""
import numpy as np
from util import gauss_window, conv_same

# bars of the metric kernel against this restatement (where they come from: tests/test_gpu_image_metrics.py)
SSIM_ATOL, SUM_RTOL, PSNR_ATOL = 2e-5, 1e-5, 1e-4


def image_metrics_np(img, target, mask=None):
    """img, target [3,H,W], mask [H,W] or None -> (mse, l1, ssim, psnr)"""
    m = 1.0 if mask is None else np.asarray(mask, np.float32).astype(np.float64)[None]
    x = np.clip(np.asarray(img, np.float32).astype(np.float64), 0.0, 1.0) * m
    y = np.asarray(target, np.float32).astype(np.float64) * m
    d = x - y
    mse, l1 = float((d * d).mean()), float(np.abs(d).mean())
    g = gauss_window()
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    mu1, mu2 = conv_same(x, g), conv_same(y, g)
    s1, s2, s12 = conv_same(x * x, g) - mu1 * mu1, conv_same(y * y, g) - mu2 * mu2, conv_same(x * y, g) - mu1 * mu2
    ssim = float((((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).mean())
    return mse, l1, ssim, -10.0 * np.log10(max(mse, 1e-10))


def assert_metrics_close(got, ref, what=""):
    """got, ref = (mse, l1, ssim, psnr); prints the figures, then holds them to the bars above"""
    print(f"{what}: got {tuple(float(v) for v in got)} ref {tuple(float(v) for v in ref)}")
    assert abs(got[0] - ref[0]) <= SUM_RTOL * ref[0], (what, "mse", got[0], ref[0])
    assert abs(got[1] - ref[1]) <= SUM_RTOL * ref[1], (what, "l1", got[1], ref[1])
    assert abs(got[2] - ref[2]) < SSIM_ATOL, (what, "ssim", got[2], ref[2])
    assert abs(got[3] - ref[3]) < PSNR_ATOL, (what, "psnr", got[3], ref[3])
