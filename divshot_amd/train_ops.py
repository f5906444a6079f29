"""ctypes wrappers of include/dvs_train.h (loss gradient, SSIM, fused Adam) and of the view calls of include/dvs_image.h on torch CUDA tensors."""
import ctypes as C
import torch
from ._lib import lib, check, AdamGroup, MetricsView, DownsampleView


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def l1_loss_grad(img, target):
    """-> (dL [like img], loss scalar tensor): mean |img - target| and its gradient."""
    dL = torch.empty_like(img)
    loss = torch.zeros(1, dtype=torch.float32, device=img.device)
    check(lib.dvs_l1_loss_grad(_st(), img.data_ptr(), target.data_ptr(), img.numel(), dL.data_ptr(), loss.data_ptr()), "dvs_l1_loss_grad")
    return dL, loss


class Ssim:
    """SSIM (11x11 Gaussian window, sigma 1.5, zero padding) of [3,H,W] images with reusable scratch maps."""

    def __init__(self, width, height, device):
        self.W, self.H = width, height
        self.maps = [torch.empty((3, height, width), dtype=torch.float32, device=device) for _ in range(3)]
        self.sum = torch.zeros(4096, dtype=torch.float32, device=device)      # DVS_SSIM_SLOTS partial sums

    def forward(self, img, target):
        """-> mean SSIM as a 1-element tensor (asynchronous)."""
        self.sum.zero_()
        check(lib.dvs_ssim_forward(_st(), img.data_ptr(), target.data_ptr(), self.W, self.H, self.maps[0].data_ptr(),
                                   self.maps[1].data_ptr(), self.maps[2].data_ptr(), self.sum.data_ptr()), "dvs_ssim_forward")
        return self.sum.sum().reshape(1) / (3.0 * self.W * self.H)

    def loss_backward(self, img, target, ssim_weight):
        """After forward(): dL of (1-w) mean|x-y| + w (1 - mean SSIM) in one pass (dvs_loss_l1_ssim_backward).
        -> (dL [3,H,W], l1 term as a 1-element tensor = (1-w) mean|x-y|)."""
        dL = torch.empty_like(img)
        l1 = torch.zeros(4096, dtype=torch.float32, device=img.device)            # DVS_SSIM_SLOTS
        check(lib.dvs_loss_l1_ssim_backward(_st(), img.data_ptr(), target.data_ptr(), self.W, self.H, self.maps[0].data_ptr(),
                                            self.maps[1].data_ptr(), self.maps[2].data_ptr(), float(ssim_weight), dL.data_ptr(), l1.data_ptr()),
              "dvs_loss_l1_ssim_backward")
        return dL, l1.sum().reshape(1)

    def backward(self, img, target, dL, scale, accumulate=True):
        """dL (+)= scale * d(mean SSIM)/d(img)."""
        check(lib.dvs_ssim_backward(_st(), img.data_ptr(), target.data_ptr(), self.W, self.H, self.maps[0].data_ptr(),
                                    self.maps[1].data_ptr(), self.maps[2].data_ptr(), float(scale), dL.data_ptr(), int(accumulate)),
              "dvs_ssim_backward")
        return dL


def image_metrics(imgs, targets, masks=None):
    """Image metrics of V views in one call (dvs_image_metrics_views) -> torch.float64 [V, 4], rows {mse, l1, ssim, psnr} (asynchronous).
    imgs: V float32 [3,H,W] tensors (or one [V,3,H,W]); targets: likewise, all float32 or all uint8; masks: None, or V entries each None
    or a float32 [H,W] tensor. The rendered view is clamped to [0, 1] and both images are multiplied by the mask (include/dvs_train.h)."""
    imgs, targets = list(imgs), list(targets)
    V = len(imgs)
    masks = [None] * V if masks is None else list(masks)
    if len(targets) != V or len(masks) != V:
        raise ValueError("image_metrics: imgs, targets and masks must have one entry per view")
    H, W = (int(d) for d in imgs[0].shape[-2:]) if V else (0, 0)
    u8 = V > 0 and targets[0].dtype == torch.uint8
    arr = (MetricsView * max(V, 1))()
    for a, x, y, m in zip(arr, imgs, targets, masks):
        if x.dtype != torch.float32 or tuple(x.shape) != (3, H, W) or not x.is_contiguous():
            raise ValueError("image_metrics: every img must be a contiguous float32 [3,H,W] tensor of one size")
        if y.dtype != (torch.uint8 if u8 else torch.float32) or tuple(y.shape) != (3, H, W) or not y.is_contiguous():
            raise ValueError("image_metrics: every target must be a contiguous [3,H,W] tensor, all float32 or all uint8")
        if m is not None and (m.dtype != torch.float32 or tuple(m.shape) != (H, W) or not m.is_contiguous()):
            raise ValueError("image_metrics: a mask must be a contiguous float32 [H,W] tensor")
        a.img, a.target, a.mask = x.data_ptr(), y.data_ptr(), m.data_ptr() if m is not None else None
    dev = imgs[0].device if V else torch.device("cuda")
    scratch = torch.empty(max(4, lib.dvs_image_metrics_scratch_bytes(W, H, V)), dtype=torch.uint8, device=dev)
    out = torch.empty((max(V, 1), 4), dtype=torch.float64, device=dev)
    check(lib.dvs_image_metrics_views(_st(), arr, V, W, H, int(u8), scratch.data_ptr(), out.data_ptr()), "dvs_image_metrics_views")
    return out[:V]


def downsample_views(srcs, factor):
    """Box downsample of V views by factor 1, 2, 4 or 8 in one call (dvs_downsample_views) -> list of V float32 [planes, H // f, W // f]
    tensors (asynchronous). srcs: V contiguous [planes, H, W] tensors of one shape, all float32 or all uint8; any element alignment."""
    srcs = list(srcs)
    V = len(srcs)
    planes, H, W = (int(d) for d in srcs[0].shape)
    u8 = srcs[0].dtype == torch.uint8
    for x in srcs:
        if x.dtype != (torch.uint8 if u8 else torch.float32) or tuple(x.shape) != (planes, H, W) or not x.is_contiguous():
            raise ValueError("downsample_views: every source must be a contiguous [planes,H,W] tensor of one shape, all float32 or all uint8")
    outs = [torch.empty((planes, H // factor, W // factor), dtype=torch.float32, device=x.device) for x in srcs]
    arr = (DownsampleView * max(V, 1))()
    for a, x, o in zip(arr, srcs, outs):
        a.src, a.dst = x.data_ptr(), o.data_ptr()
    check(lib.dvs_downsample_views(_st(), arr, V, planes, W, H, int(factor), int(u8)), "dvs_downsample_views")
    return outs


def undistort_view(src, desc, mask=None):
    """A distorted camera's view as its pinhole camera sees it (dvs_undistort_view) -> (dst uint8 [planes,H,W], mask float32 [H,W],
    invalid: int32 1-element tensor, the number of pixels without a source) (asynchronous). src: contiguous uint8 [planes,H,W], planes
    1..4; desc: _lib.UndistortDesc (undistort_desc()); mask: None or a contiguous uint8 [H,W] tensor of 0 / 1 in the source's geometry."""
    if src.dtype != torch.uint8 or src.dim() != 3 or not src.is_contiguous() or tuple(src.shape[1:]) != (desc.height, desc.width):
        raise ValueError("undistort_view: src must be a contiguous uint8 [planes,H,W] tensor of the descriptor's size")
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != tuple(src.shape[1:]) or not mask.is_contiguous()):
        raise ValueError("undistort_view: mask must be a contiguous uint8 [H,W] tensor")
    dst = torch.empty_like(src)
    out_mask = torch.empty(tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
    invalid = torch.zeros(1, dtype=torch.int32, device=src.device)
    check(lib.dvs_undistort_view(_st(), C.byref(desc), int(src.shape[0]), src.data_ptr(), mask.data_ptr() if mask is not None else None,
                                 dst.data_ptr(), out_mask.data_ptr(), invalid.data_ptr()), "dvs_undistort_view")
    return dst, out_mask, invalid


def adam_step(param, grad, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-15):
    check(lib.dvs_adam_step(_st(), param.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), param.numel(), float(lr), float(beta1),
                            float(beta2), float(eps), int(step)), "dvs_adam_step")


def adam_step_groups(groups, step, beta1=0.9, beta2=0.999, eps=1e-15, visible=None):
    """All parameter groups in one launch. groups: iterable of dicts {param, grad, m, v, lr, width[, tiled, active_chunks]};
    visible: optional int32 [n] radii tensor -> only splats with radii > 0 are updated (the reference's visibleAdam)."""
    arr = (AdamGroup * len(groups))()
    for a, g in zip(arr, groups):
        a.param, a.grad, a.m, a.v = g["param"].data_ptr(), g["grad"].data_ptr(), g["m"].data_ptr(), g["v"].data_ptr()
        a.count, a.lr, a.width = g["param"].numel(), float(g["lr"]), int(g["width"])
        a.layout, a.active_chunks = int(bool(g.get("tiled", False))), int(g.get("active_chunks", 0))
    check(lib.dvs_adam_step_groups(_st(), arr, len(groups), float(beta1), float(beta2), float(eps), int(step),
                                   visible.data_ptr() if visible is not None else None, int(visible.numel()) if visible is not None else 0),
          "dvs_adam_step_groups")
