"""3D smoothing filter (the world-space half of Mip-Splatting) — Python handles over the last section of include/dvs_train.h.

torch supplies device buffers and the HIP stream; all compute runs in libdvsraster.so:
    rows = pack_cameras(cameras)                                   # host only: [n_cams,16] float32
    filt, info = compute(pos, cameras)                             # cameras: a list of Camera, or packed rows; info = {"max", "n_seen"}
    scale_eff, opacity_eff = apply(scale, opacity, filt)           # first / count: only that range of rows is written
    chain(scale, opacity, filt, g_scale, g_opacity)                # in place
All tensors are contiguous float32 device tensors: pos [n,3], scale [n,3], opacity [n], filt [n].
"""
import ctypes as C
import numpy as np
import torch
from ._lib import lib, Camera, DvsError, check
from .raster import _stream_ptr


def pack_cameras(cameras):
    """dvs_filter3d_pack_cameras: a list of Camera -> float32 [n_cams,16] (three rows of world-to-camera, focal_x, width, height, pad)"""
    cams = (Camera * len(cameras))(*cameras)
    rows = np.zeros((len(cameras), 16), np.float32)
    if lib.dvs_filter3d_pack_cameras(cams, len(cameras), rows.ctypes.data) != 0:
        raise DvsError("dvs_filter3d_pack_cameras refused the cameras")
    return rows


def _f32(t, what):
    if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
        raise DvsError(f"filter3d: {what} must be a contiguous float32 device tensor")
    return t


def compute(pos, cameras):
    """-> (filter [n], {"max": the maximum over the seen splats, "n_seen": how many splats some camera sees})"""
    _f32(pos, "pos")
    n = pos.numel() // 3
    rows = cameras if isinstance(cameras, np.ndarray) else pack_cameras(cameras)
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 16)
    dev = pos.device
    with torch.cuda.device(dev):
        d_rows = torch.from_numpy(rows).to(dev)
        filt = torch.empty(max(n, 1), device=dev)[:n]
        scratch = torch.zeros(4, dtype=torch.int32, device=dev)
        check(lib.dvs_filter3d_compute(_stream_ptr(), n, pos.data_ptr(), d_rows.data_ptr(), rows.shape[0], filt.data_ptr(), scratch.data_ptr()),
              "dvs_filter3d_compute")
        s = scratch.cpu().numpy()                                            # (synchronises: d_rows leaves scope)
    return filt, {"max": float(s[:1].view(np.float32)[0]), "n_seen": int(s[1:2].view(np.uint32)[0])}


def apply(scale, opacity, filt, first=0, count=None, out=None):
    """-> (scale_eff [n,3], opacity_eff [n]); with first / count only the rows [first, first + count) are written (out: the tensors to write)"""
    n = opacity.numel()
    count = n - first if count is None else count
    for t, what in ((scale, "scale"), (opacity, "opacity"), (filt, "filter")):
        _f32(t, what)
    scale_eff, opacity_eff = out if out is not None else (torch.empty_like(scale), torch.empty_like(opacity))
    with torch.cuda.device(scale.device):
        check(lib.dvs_filter3d_apply_range(_stream_ptr(), n, int(first), int(count), scale.data_ptr(), opacity.data_ptr(), filt.data_ptr(),
                                           _f32(scale_eff, "scale_eff").data_ptr(), _f32(opacity_eff, "opacity_eff").data_ptr()), "dvs_filter3d_apply_range")
    return scale_eff, opacity_eff


def chain(scale, opacity, filt, g_scale, g_opacity, first=0, count=None):
    """g_scale [n,3], g_opacity [n]: gradients with respect to the effective values -> with respect to the trained ones, in place"""
    n = opacity.numel()
    count = n - first if count is None else count
    for t, what in ((scale, "scale"), (opacity, "opacity"), (filt, "filter"), (g_scale, "g_scale"), (g_opacity, "g_opacity")):
        _f32(t, what)
    with torch.cuda.device(scale.device):
        check(lib.dvs_filter3d_chain_range(_stream_ptr(), n, int(first), int(count), scale.data_ptr(), opacity.data_ptr(), filt.data_ptr(),
                                           g_scale.data_ptr(), g_opacity.data_ptr()), "dvs_filter3d_chain_range")
    return g_scale, g_opacity
