"""Level-of-detail export — Python handles over the last section of include/dvs_export.h.

torch supplies device buffers and the HIP stream; all compute runs in libdvsraster.so:
    lat = lattice_for(bounds, resolution)                          # host only: {min xyz, max xyz} -> LodLattice
    out, counts = merge_splats(params, lattice=lat, sh_degree=3)   # or bounds=..., resolution=...
params / out: dicts of float32 device tensors pos [n,3], sh0 [n,3], shN, opacity [n], scale [n,3], rot [n,4]; shN in DVS_SHN_ROWS [n,45]
(layout 0) or DVS_SHN_TILED (1: whole 64-splat tiles of 48 floats). counts = {"m": ..., "n_dropped": ...}.
"""
import ctypes as C
import numpy as np
import torch
from ._lib import lib, LodLattice, DvsError, check
from .raster import _stream_ptr

KEYS = ("pos", "sh0", "shN", "opacity", "scale", "rot")


def make_lattice(origin, cell, dims):
    """-> LodLattice from its parts (not checked here: the entry points refuse what is not a lattice)"""
    g = LodLattice()
    g.origin[:] = [float(v) for v in np.asarray(origin, np.float32).reshape(3)]
    g.cell = float(np.float32(cell))
    g.dims[:] = [int(v) for v in dims]
    return g


def lattice_for(bounds, resolution):
    """bounds = {min xyz, max xyz} -> the LodLattice of dvs_lod_lattice_for; DvsError when it is refused"""
    b = np.ascontiguousarray(bounds, np.float32).reshape(6)
    g = LodLattice()
    if lib.dvs_lod_lattice_for(b.ctypes.data, int(resolution), C.byref(g)) != 0:
        raise DvsError(f"dvs_lod_lattice_for refused bounds {b.tolist()}, resolution {resolution}")
    return g


def finite_bounds(pos):
    """{min xyz, max xyz} over the rows of pos (a device tensor [n,3]) whose three coordinates are finite; DvsError when there is none"""
    ok = torch.isfinite(pos).all(dim=1)
    if not bool(ok.any()):
        raise DvsError("no splat has a finite centre")
    p = pos[ok]
    return torch.cat([p.min(dim=0).values, p.max(dim=0).values]).cpu().numpy()


def merge_splats(params, lattice=None, bounds=None, resolution=None, sh_degree=3, shn_layout=0, shn_layout_out=None, n=None, out=None):
    """The model merged on `lattice` (or on lattice_for(bounds, resolution); bounds None: the bounds of the finite centres).
    n: the splat count (needed with a tiled shN whose tensor holds whole tiles). out: None (new tensors), or a dict of tensors to write
    with room for the result (n rows always are enough; tiled shN: whole tiles). -> (out, counts): out in shn_layout_out (default:
    shn_layout), cut to m rows each (tiled shN: ceil(m / 64) tiles)."""
    pos = params["pos"]
    n = pos.numel() // 3 if n is None else int(n)
    shn_layout_out = shn_layout if shn_layout_out is None else shn_layout_out
    dev = pos.device
    if lattice is None:
        if resolution is None:
            raise DvsError("merge_splats needs a lattice or a resolution")
        lattice = lattice_for(finite_bounds(pos[:n]) if bounds is None else bounds, resolution)
    ptr = lambda a: None if a is None else a.data_ptr()
    counts = (C.c_uint32 * 2)()
    with torch.cuda.device(dev):
        scratch = torch.empty(lib.dvs_lod_scratch_bytes(n) + 256, dtype=torch.uint8, device=dev)
        sp = (scratch.data_ptr() + 255) & ~255
        check(lib.dvs_lod_merge_count(_stream_ptr(), n, ptr(pos), ptr(params["opacity"]), ptr(params["scale"]), ptr(params["rot"]), C.byref(lattice), sp,
                                      counts), "dvs_lod_merge_count")
        m = int(counts[0])
        rows = max(m, 1)                                                     # (an empty tensor has no address)
        tiled_floats = ((rows + 63) // 64) * 64 * 48
        if out is None:
            out = {"pos": torch.empty(rows, 3, device=dev), "sh0": torch.empty(rows, 3, device=dev),
                   "shN": torch.empty((tiled_floats,) if shn_layout_out == 1 else (rows, 45), device=dev), "opacity": torch.empty(rows, device=dev),
                   "scale": torch.empty(rows, 3, device=dev), "rot": torch.empty(rows, 4, device=dev)}
        else:
            need = {"pos": rows * 3, "sh0": rows * 3, "shN": tiled_floats if shn_layout_out == 1 else rows * 45, "opacity": rows, "scale": rows * 3, "rot": rows * 4}
            for k in KEYS:
                if out[k].numel() < need[k] or not out[k].is_contiguous() or out[k].dtype != torch.float32:
                    raise DvsError(f"merge_splats: out['{k}'] has no room for {m} rows as contiguous float32")
        check(lib.dvs_lod_merge_write(_stream_ptr(), n, int(sh_degree), *[ptr(params[k]) for k in KEYS], int(shn_layout), sp,
                                      *[ptr(out[k]) for k in KEYS], int(shn_layout_out)), "dvs_lod_merge_write")
        torch.cuda.synchronize(dev)                                          # (the scratch leaves scope)
    cut = {}
    for k, w in (("pos", 3), ("sh0", 3), ("shN", 45), ("opacity", 1), ("scale", 3), ("rot", 4)):
        flat = out[k].reshape(-1)
        if k == "shN" and shn_layout_out == 1:
            cut[k] = flat[:((m + 63) // 64) * 64 * 48]
        else:
            cut[k] = flat[:m * w].reshape((m, w) if w > 1 else (m,))
    return cut, {"m": m, "n_dropped": int(counts[1])}
