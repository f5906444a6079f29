"""Focus region — Python handles over include/dvs_region.h.

torch supplies device buffers and the HIP stream; all compute runs in libdvsraster.so:
    region, b2w = region_from_trs(pos, rot, scale, lo, hi)        # host only
    action, offsets, new_count = region_plan(pos, region)          # what dvs_densify_apply compacts from
    region_mask_views(cams, region, outs, in_masks)                # outs[v] = in_masks[v] * hit
"""
import ctypes as C
import numpy as np
import torch
from ._lib import lib, Region, RegionMaskView, DvsError, check
from .raster import _stream_ptr


def region_from_trs(pos, rot, scale, lo, hi):
    """-> (Region, b2w float32 [4,4] row-major = F) of dvs_region_from_trs; DvsError when it refuses"""
    v = [np.ascontiguousarray(a, np.float32).reshape(3) for a in (pos, rot, scale, lo, hi)]
    region, b2w = Region(), np.zeros((4, 4), np.float32)
    if lib.dvs_region_from_trs(*[a.ctypes.data for a in v], C.byref(region), b2w.ctypes.data) != 0:
        raise DvsError(f"dvs_region_from_trs refused pos {pos}, rot {rot}, scale {scale}, lo {lo}, hi {hi}")
    return region, b2w


def region_plan(pos, region):
    """pos: float32 tensor on the device whose first 3 n floats are the centres (any alignment); -> (action uint8 [n], offsets int32 [n],
    new_count int): action 0 (DVS_DENSIFY_KEEP) inside the region, 3 (DVS_DENSIFY_PRUNE) outside; offsets = the exclusive scan of the kept"""
    assert pos.is_cuda and pos.dtype == torch.float32 and pos.is_contiguous() and pos.numel() % 3 == 0
    n = pos.numel() // 3
    action = torch.empty(n, dtype=torch.uint8, device=pos.device)
    offsets = torch.empty(n, dtype=torch.int32, device=pos.device)
    new_count = torch.full((1,), -1, dtype=torch.int64, device=pos.device)
    scratch = torch.empty(n // 256 + 2, dtype=torch.int32, device=pos.device)
    with torch.cuda.device(pos.device):
        check(lib.dvs_region_plan(_stream_ptr(), n, pos.data_ptr(), C.byref(region), action.data_ptr(), offsets.data_ptr(), scratch.data_ptr(),
                                  new_count.data_ptr()), "dvs_region_plan")
    return action, offsets, int(new_count.item())


def region_mask_views(cams, region, outs, in_masks=None):
    """cams: list of Camera, all width x height; outs: one float32 device tensor of H * W floats per view (any alignment), written;
    in_masks: None, or one entry per view, each None or such a tensor"""
    V = len(cams)
    views = (RegionMaskView * V)()
    for v in range(V):
        assert outs[v].is_cuda and outs[v].dtype == torch.float32 and outs[v].is_contiguous()
        views[v].cam = cams[v]
        m = in_masks[v] if in_masks is not None else None
        views[v].in_mask = None if m is None else m.data_ptr()
        views[v].out = outs[v].data_ptr()
    with torch.cuda.device(outs[0].device):
        check(lib.dvs_region_mask_views(_stream_ptr(), views, V, cams[0].width, cams[0].height, C.byref(region)), "dvs_region_mask_views")
