"""Shared helpers for the parity tests."""
import numpy as np
import divshot_amd as dv

KEYS = ("pos", "sh0", "shN", "opacity", "scale", "rot")


def scene(n, w, h, deg=3, seed=1, n_cams=1, cam_index=0, scale_offset=0.0, bg=(0.0, 0.0, 0.0)):
    spec = dv.make_spec(n, w, h, sh_degree=deg, seed=seed, n_cams=n_cams, scale_log_offset=scale_offset)
    P = dv.synth_splats(spec)
    cam = dv.synth_camera(spec, cam_index)
    for k in range(3):
        cam.bg[k] = bg[k]
    tgt = dv.synth_target(spec, cam_index)
    return spec, P, cam, tgt


def rel_close(a, ref, rtol, atol_frac):
    """|a-ref| <= rtol*|ref| + atol_frac*max|ref|  ->  (ok mask, worst normalised error)"""
    a = np.asarray(a, np.float64); ref = np.asarray(ref, np.float64)
    scale = np.abs(ref).max() if ref.size else 0.0
    tol = rtol * np.abs(ref) + atol_frac * scale
    err = np.abs(a - ref)
    worst = float((err / np.maximum(tol, 1e-300)).max()) if ref.size else 0.0
    return err <= tol, worst


# ---- restatements shared by the training-op tests (tests/test_gpu_train_ops*.py) ----------------------------------------------
def gauss_window():
    """the 11-tap SSIM window, sigma 1.5, normalised (fp64)"""
    x = np.arange(11) - 5.0
    g = np.exp(-x * x / (2 * 1.5 ** 2))
    return g / g.sum()


def conv_same(img, g):
    """separable 11-tap convolution with zero padding over the last two axes, img [..., H, W] float64"""
    H, W = img.shape[-2:]
    pad = [(0, 0)] * (img.ndim - 2) + [(5, 5), (5, 5)]
    p = np.pad(img, pad)
    t = sum(g[k] * p[..., :, k:k + W] for k in range(11))
    return sum(g[k] * t[..., k:k + H, :] for k in range(11))


def relocation_np(o, ratio, min_opacity):
    """numpy restatement of the MCMC relocation rule (opacity / scale of the c+1 copies of a splat drawn c times): o may be an
    array (one ratio for all of it)."""
    from math import comb, sqrt
    no = 1.0 - (1.0 - o) ** (1.0 / ratio)
    denom = sum(comb(i - 1, k) * (-1) ** k * no ** (k + 1) / sqrt(k + 1) for i in range(1, ratio + 1) for k in range(i))
    return np.clip(no, min_opacity, 1.0 - 1.1920929e-7), o / denom
