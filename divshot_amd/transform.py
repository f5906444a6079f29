"""Export in a chosen frame — Python handles over the last section of include/dvs_export.h.

torch supplies device buffers and the HIP stream; all compute runs in libdvsraster.so:
    sim = similarity_from_trs(t, euler_rad, s)                    # host only: p' = s R p + t, R = Rz Ry Rx
    inv = similarity_inverse(sim)                                  # host only
    D = sh_rotation(sim.R)                                         # host only: float32 [83], the 3x3, 5x5, 7x7 band matrices
    pos, shN, scale, rot = transform_splats(sim, D, pos, shN, scale, rot, sh_degree, layout)     # new tensors, or in place
    xyz, normals = transform_points(sim, xyz, normals)
"""
import ctypes as C
import numpy as np
import torch
from ._lib import lib, Similarity, DvsError, check, host_lib
from .raster import _stream_ptr


def make_similarity(R, t, s):
    """-> Similarity from a row-major 3x3 R, t [3] and s (not checked here: the entry points refuse what is not a similarity)"""
    m = Similarity()
    m.R[:] = [float(v) for v in np.asarray(R, np.float32).reshape(9)]
    m.t[:] = [float(v) for v in np.asarray(t, np.float32).reshape(3)]
    m.s = float(np.float32(s))
    return m


def similarity_from_trs(t, euler_rad, s):
    v = [np.ascontiguousarray(a, np.float32).reshape(3) for a in (t, euler_rad)]
    m = Similarity()
    if lib.dvs_similarity_from_trs(v[0].ctypes.data, v[1].ctypes.data, float(s), C.byref(m)) != 0:
        raise DvsError(f"dvs_similarity_from_trs refused t {t}, euler {euler_rad}, s {s}")
    return m


def similarity_inverse(sim):
    m = Similarity()
    if lib.dvs_similarity_inverse(C.byref(sim), C.byref(m)) != 0:
        raise DvsError("dvs_similarity_inverse refused its input")
    return m


def sh_rotation(R):
    """-> float32 [83]: the band matrices of dvs_sh_rotation for the row-major 3x3 R; DvsError when R is not a rotation"""
    R = np.ascontiguousarray(R, np.float32).reshape(9)
    D = np.zeros(83, np.float32)
    if lib.dvs_sh_rotation(R.ctypes.data, D.ctypes.data) != 0:
        raise DvsError(f"dvs_sh_rotation refused R {R.tolist()}")
    return D


def transform_splats(sim, D, pos, shN, scale, rot, sh_degree, shn_layout=0, n=None, out=None):
    """pos [n,3], scale [n,3], rot [n,4] float32 device tensors; shN in DVS_SHN_ROWS [n,45] (shn_layout 0) or DVS_SHN_TILED (1, whole
    tiles; pass n), or None at degree 0. out: None (new tensors), "inplace", or a tuple (pos, shN, scale, rot) of tensors to write.
    -> (pos, shN, scale, rot) as written"""
    n = pos.numel() // 3 if n is None else int(n)
    D = np.ascontiguousarray(D, np.float32).reshape(83)
    if out is None:
        out = tuple(None if a is None else torch.empty_like(a) for a in (pos, shN, scale, rot))
    elif isinstance(out, str):
        out = (pos, shN, scale, rot)
    ptr = lambda a: None if a is None else a.data_ptr()
    with torch.cuda.device(pos.device):
        check(lib.dvs_transform_splats(_stream_ptr(), n, int(sh_degree), C.byref(sim), D.ctypes.data, ptr(pos), ptr(shN), int(shn_layout), ptr(scale),
                                       ptr(rot), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3])), "dvs_transform_splats")
    return out


def transform_points(sim, xyz, normals=None, inplace=False):
    """xyz, normals: float32 device tensors [n,3] (normals may be None) -> (xyz', normals')"""
    n = xyz.numel() // 3
    xo = xyz if inplace else torch.empty_like(xyz)
    no = None if normals is None else (normals if inplace else torch.empty_like(normals))
    with torch.cuda.device(xyz.device):
        check(lib.dvs_transform_points(_stream_ptr(), n, C.byref(sim), xyz.data_ptr(), None if normals is None else normals.data_ptr(), xo.data_ptr(),
                                       None if no is None else no.data_ptr()), "dvs_transform_points")
    return xo, no


def export_orientation(views, centres, axis):
    """gsframe::orientation through libgsplyio.so (host only): views float32 [n,16] (dvs_camera.view), centres float32 [n,3], axis "+y" ...
    -> (R float64 [3,3], t float64 [3]) with s = 1; DvsError with the reason when it is refused"""
    views = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
    centres = np.ascontiguousarray(centres, np.float32).reshape(-1, 3)
    R, t = np.zeros(9, np.float64), np.zeros(3, np.float64)
    err = C.create_string_buffer(512)
    if host_lib().gstrain_export_orientation(len(views), views.ctypes.data, centres.ctypes.data, axis.encode(), R.ctypes.data, t.ctypes.data, err, 512) != 0:
        raise DvsError(err.value.decode(errors="replace"))
    return R.reshape(3, 3), t
