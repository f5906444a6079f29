"""Importance-scored pruning and the mask carve — Python handles over dvs_raster_importance_views / dvs_raster_foreground_views
(include/dvs_raster.h) and dvs_importance_plan / dvs_foreground_plan (include/dvs_train.h).

torch supplies device buffers and the HIP stream; all compute runs in libdvsraster.so:
    score, wmax, hits = importance_scores(rasterizer)            # of the rasterizer's last forward / forward_views
    importance_scores(rasterizer, out=(score, wmax, hits))       # ... accumulated into the arrays of an earlier call
    action, offsets, new_count = importance_plan(score, keep)    # what dvs_densify_apply compacts from
    fg, bg = foreground_votes(rasterizer, fg_masks, valid_masks) # where that blend weight landed: foreground / background pixels
    action, offsets, new_count = foreground_plan(fg, bg, 50)     # keeps the splats the foreground voted for
"""
import ctypes as C
import torch
from ._lib import lib, Opts, check
from .raster import _stream_ptr


def _mask_array(rasterizer, masks):
    """None, or the HOST array of DEVICE pointers the view passes take: one entry per view, each None or a [H,W] float32 tensor"""
    if masks is None:
        return None
    cams = getattr(rasterizer, "_cams", None)
    V = len(cams) if cams is not None else 1
    assert len(masks) == V, (len(masks), V)
    H, W = rasterizer._cam.height, rasterizer._cam.width
    for k in masks:
        assert k is None or (k.is_cuda and k.dtype == torch.float32 and k.is_contiguous() and tuple(k.shape) == (H, W))
    return (C.c_void_p * V)(*[None if k is None else k.data_ptr() for k in masks])


def importance_scores(rasterizer, masks=None, out=None):
    """-> (sum, max, hits) per splat of the last forward on `rasterizer`, torch tensors [n] on its device: sum int64 (the uint64 sum of
    rintf(w * 2^24), w = alpha T, over the (view, pixel) pairs that took the splat), max float32 (the largest w), hits int32 (the number
    of those pairs). masks: None, or one entry per view, each None or a [H,W] float32 tensor (a pixel with mask 0 contributes nothing).
    out: the triple of an earlier call to accumulate into (the call adds to what the arrays hold; fresh arrays are zeroed here).
    DvsError (DVS_ERR_STATE) when the context holds no forward."""
    st = rasterizer.state
    n = int(st.n) if st is not None else 1
    if out is None:
        out = (torch.zeros(n, dtype=torch.int64, device=rasterizer.tdev), torch.zeros(n, dtype=torch.float32, device=rasterizer.tdev),
               torch.zeros(n, dtype=torch.int32, device=rasterizer.tdev))
    s, m, h = out
    for t, dt in ((s, torch.int64), (m, torch.float32), (h, torch.int32)):
        assert t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == n, (t.dtype, t.numel(), n)
    mask_arr = _mask_array(rasterizer, masks)
    opts = rasterizer._opts if rasterizer._opts is not None else Opts()
    with torch.cuda.device(rasterizer.tdev):
        check(lib.dvs_raster_importance_views(rasterizer.ctx, _stream_ptr(), C.byref(opts), mask_arr, s.data_ptr(), m.data_ptr(), h.data_ptr()),
              "dvs_raster_importance_views")
    return s, m, h


def importance_plan(score, keep):
    """score: int64 tensor [n] on the device (importance_scores' sum, read as uint64); keep: how many splats stay (> n keeps all).
    -> (action uint8 [n], offsets int32 [n], new_count int): the n - min(keep, n) splats smallest in (score, then larger index first)
    are DVS_DENSIFY_PRUNE (3), the others DVS_DENSIFY_KEEP (0); offsets = the exclusive scan of the kept; new_count = min(keep, n)."""
    assert score.is_cuda and score.dtype == torch.int64 and score.is_contiguous() and score.dim() == 1
    n = score.numel()
    action = torch.empty(n, dtype=torch.uint8, device=score.device)
    offsets = torch.empty(n, dtype=torch.int32, device=score.device)
    new_count = torch.zeros(1, dtype=torch.int64, device=score.device)
    scratch = torch.empty(max(int(lib.dvs_importance_scratch_bytes(n)), 16), dtype=torch.uint8, device=score.device)
    with torch.cuda.device(score.device):
        check(lib.dvs_importance_plan(_stream_ptr(), n, score.data_ptr(), int(keep), action.data_ptr(), offsets.data_ptr(), scratch.data_ptr(),
                                      new_count.data_ptr()), "dvs_importance_plan")
    return action, offsets, int(new_count.item())


def foreground_votes(rasterizer, fg_masks=None, valid_masks=None, out=None):
    """-> (fg, bg) per splat of the last forward on `rasterizer`, int64 tensors [n] on its device (read as uint64): the sum of
    rintf(w * 2^24), w = alpha T, over the (view, pixel) pairs that took the splat, split by the pixel's label — fg where the view's
    fg mask is nonzero (or the view has none), bg elsewhere. A pixel whose valid mask is 0 walks nothing. fg + bg equals
    importance_scores(masks=valid_masks)' sum bit for bit. Both mask lists: None, or one entry per view, each None or a [H,W] float32
    tensor. out: the pair of an earlier call to accumulate into (fresh arrays are zeroed here). DvsError (DVS_ERR_STATE) when the
    context holds no forward."""
    st = rasterizer.state
    n = int(st.n) if st is not None else 1
    if out is None:
        out = (torch.zeros(n, dtype=torch.int64, device=rasterizer.tdev), torch.zeros(n, dtype=torch.int64, device=rasterizer.tdev))
    fg, bg = out
    for t in (fg, bg):
        assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.numel() == n, (t.dtype, t.numel(), n)
    fg_arr, valid_arr = _mask_array(rasterizer, fg_masks), _mask_array(rasterizer, valid_masks)
    opts = rasterizer._opts if rasterizer._opts is not None else Opts()
    with torch.cuda.device(rasterizer.tdev):
        check(lib.dvs_raster_foreground_views(rasterizer.ctx, _stream_ptr(), C.byref(opts), fg_arr, valid_arr, fg.data_ptr(), bg.data_ptr()),
              "dvs_raster_foreground_views")
    return fg, bg


def foreground_plan(fg, bg, percent):
    """fg, bg: int64 tensors [n] on the device (foreground_votes' sums, read as uint64); percent: 1..100.
    -> (action uint8 [n], offsets int32 [n], new_count int): splat i is DVS_DENSIFY_KEEP (0) iff fg[i] > 0 and
    fg[i] * (100 - percent) >= bg[i] * percent (exact for every 64-bit input), else DVS_DENSIFY_PRUNE (3); offsets = the exclusive
    scan of the kept; new_count = their number."""
    assert fg.is_cuda and fg.dtype == torch.int64 and fg.is_contiguous() and fg.dim() == 1
    assert bg.is_cuda and bg.dtype == torch.int64 and bg.is_contiguous() and bg.shape == fg.shape and bg.device == fg.device
    n = fg.numel()
    action = torch.empty(n, dtype=torch.uint8, device=fg.device)
    offsets = torch.empty(n, dtype=torch.int32, device=fg.device)
    new_count = torch.zeros(1, dtype=torch.int64, device=fg.device)
    scratch = torch.empty(n // 256 + 4, dtype=torch.int32, device=fg.device)
    with torch.cuda.device(fg.device):
        check(lib.dvs_foreground_plan(_stream_ptr(), n, fg.data_ptr(), bg.data_ptr(), int(percent), action.data_ptr(), offsets.data_ptr(),
                                      scratch.data_ptr(), new_count.data_ptr()), "dvs_foreground_plan")
    return action, offsets, int(new_count.item())
