"""Surface extraction — Python handles over include/dvs_mesh.h and dvs_raster_depth_views (include/dvs_raster.h).

torch supplies device buffers and the HIP stream; all compute runs in libdvsraster.so:
    depth, alpha = depth_maps(rasterizer)              # of the rasterizer's last forward / forward_views
    grid = TsdfGrid((x0, y0, z0), voxel, (nx, ny, nz)); grid.integrate(cams, depth, alpha, rgb, trunc=4 * voxel)
    xyz, rgb, tri = grid.extract()                      # numpy: float32 [nv,3], uint8 [nv,3], uint32 [nt,3]
    xyz, rgb, tri, nrm = grid.extract(normals=True)     # ... and the TSDF gradient's unit normals, float32 [nv,3]
    xyz, rgb, tri, nrm, info = clean_mesh(xyz, rgb, tri, min_bp=100, normals=nrm)   # components below 1 % of the largest dropped
    xyz, rgb, tri, nrm, info = decimate_mesh(xyz, rgb, tri, origin, cell, (cx, cy, cz), normals=nrm)   # one vertex per lattice cell
"""
import ctypes as C
import numpy as np
import torch
from ._lib import lib, Camera, Opts, TsdfGridDesc, MeshCleanInfo, MeshDecimateInfo, check, DvsError, write_mesh_ply  # noqa: F401
from .raster import _stream_ptr


def depth_maps(rasterizer):
    """-> (depth, alpha), torch float32 [n_views, H, W], of the last forward on `rasterizer` (dvs_raster_depth_views); DvsError
    (DVS_ERR_STATE) when the context holds no forward"""
    cams = getattr(rasterizer, "_cams", None)
    cam = getattr(rasterizer, "_cam", None)
    V = len(cams) if cams is not None else 1
    H, W = (cam.height, cam.width) if cam is not None else (1, 1)
    depth = torch.empty((V, H, W), dtype=torch.float32, device=rasterizer.tdev)
    alpha = torch.empty_like(depth)
    opts = rasterizer._opts if rasterizer._opts is not None else Opts()
    with torch.cuda.device(rasterizer.tdev):
        check(lib.dvs_raster_depth_views(rasterizer.ctx, _stream_ptr(), C.byref(opts), depth.data_ptr(), alpha.data_ptr()), "dvs_raster_depth_views")
    return depth, alpha


class TsdfGrid:
    """A dvs_tsdf_grid over torch tensors: voxel (i, j, k) centred at origin + (i, j, k) * voxel; tsdf, weight [nz, ny, nx] and
    rgb [nz, ny, nx, 3] (x fastest), cleared to tsdf 1, weight 0"""

    def __init__(self, origin, voxel, dims, device=0):
        self.tdev = torch.device("cuda", device)
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 3 or lib.dvs_tsdf_bytes((C.c_int32 * 3)(*self.dims)) == 0 or not float(voxel) > 0:
            raise DvsError(f"TsdfGrid: dims {self.dims} / voxel {voxel} refused (each dimension 2..1024, voxel > 0)")
        nx, ny, nz = self.dims
        self.tsdf = torch.empty((nz, ny, nx), dtype=torch.float32, device=self.tdev)
        self.weight = torch.empty((nz, ny, nx), dtype=torch.float32, device=self.tdev)
        self.rgb = torch.empty((nz, ny, nx, 3), dtype=torch.float32, device=self.tdev)
        self.desc = TsdfGridDesc((C.c_float * 3)(*[float(v) for v in origin]), float(voxel), (C.c_int32 * 3)(*self.dims), 0,
                                 self.tsdf.data_ptr(), self.weight.data_ptr(), self.rgb.data_ptr())
        self.clear()

    def clear(self):
        with torch.cuda.device(self.tdev):
            check(lib.dvs_tsdf_clear(_stream_ptr(), C.byref(self.desc)), "dvs_tsdf_clear")

    def upload(self, tsdf, weight, rgb=None):
        """numpy arrays [nz, ny, nx] (rgb [nz, ny, nx, 3], default: unchanged) into the grid"""
        self.tsdf.copy_(torch.from_numpy(np.ascontiguousarray(tsdf, np.float32)).reshape(self.tsdf.shape))
        self.weight.copy_(torch.from_numpy(np.ascontiguousarray(weight, np.float32)).reshape(self.weight.shape))
        if rgb is not None:
            self.rgb.copy_(torch.from_numpy(np.ascontiguousarray(rgb, np.float32)).reshape(self.rgb.shape))

    def download(self):
        """-> (tsdf, weight, rgb) as numpy"""
        return self.tsdf.cpu().numpy(), self.weight.cpu().numpy(), self.rgb.cpu().numpy()

    def integrate(self, cams, depth, alpha, rgb, trunc, masks=None):
        """fuses the views (<= 16 per call, in order): cams a list of Camera; depth, alpha [V,H,W], rgb [V,3,H,W] torch tensors on the
        device; masks None or a list of [H,W] tensors / None"""
        V = len(cams)
        H, W = int(depth.shape[-2]), int(depth.shape[-1])
        for t, shape in ((depth, (V, H, W)), (alpha, (V, H, W)), (rgb, (V, 3, H, W))):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape, (tuple(t.shape), shape)
        cam_arr = (Camera * V)(*cams)
        mask_arr = None
        if masks is not None:
            assert len(masks) == V
            for m in masks:
                assert m is None or (m.is_cuda and m.dtype == torch.float32 and m.is_contiguous() and tuple(m.shape) == (H, W))
            mask_arr = (C.c_void_p * V)(*[None if m is None else m.data_ptr() for m in masks])
        with torch.cuda.device(self.tdev):
            check(lib.dvs_tsdf_integrate(_stream_ptr(), C.byref(self.desc), cam_arr, V, depth.data_ptr(), alpha.data_ptr(), rgb.data_ptr(),
                                         mask_arr, W, H, float(trunc)), "dvs_tsdf_integrate")

    def extract(self, normals=False):
        """marching tetrahedra over the grid -> (xyz float32 [nv,3], rgb uint8 [nv,3], tri uint32 [nt,3]) as numpy; with normals=True a
        fourth array, the unit normals float32 [nv,3] of dvs_mesh_extract_normals"""
        dims = (C.c_int32 * 3)(*self.dims)
        scratch = torch.empty(lib.dvs_mesh_scratch_bytes(dims) + 256, dtype=torch.uint8, device=self.tdev)
        sp = (scratch.data_ptr() + 255) & ~255
        nv, nt = C.c_uint32(0), C.c_uint32(0)
        with torch.cuda.device(self.tdev):
            check(lib.dvs_mesh_extract_count(_stream_ptr(), C.byref(self.desc), sp, C.byref(nv), C.byref(nt)), "dvs_mesh_extract_count")
            xyz = torch.empty((max(nv.value, 1), 3), dtype=torch.float32, device=self.tdev)
            rgb = torch.empty((max(nv.value, 1), 3), dtype=torch.uint8, device=self.tdev)
            tri = torch.empty((max(nt.value, 1), 3), dtype=torch.int32, device=self.tdev)
            check(lib.dvs_mesh_extract_write(_stream_ptr(), C.byref(self.desc), sp, xyz.data_ptr(), rgb.data_ptr(), tri.data_ptr()), "dvs_mesh_extract_write")
            if normals:
                nrm = torch.empty((max(nv.value, 1), 3), dtype=torch.float32, device=self.tdev)
                check(lib.dvs_mesh_extract_normals(_stream_ptr(), C.byref(self.desc), sp, nrm.data_ptr()), "dvs_mesh_extract_normals")
            torch.cuda.synchronize()
        out = (xyz[:nv.value].cpu().numpy(), rgb[:nv.value].cpu().numpy(), tri[:nt.value].cpu().numpy().view(np.uint32))
        return out + (nrm[:nv.value].cpu().numpy(),) if normals else out


def _tri_to_device(tri, device):
    tri = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    d = torch.empty((max(len(tri), 1), 3), dtype=torch.int32, device=device)
    if len(tri):
        d[:len(tri)].copy_(torch.from_numpy(tri.view(np.int32)))
    return tri, d


def mesh_components(tri, n_vertices, device=0):
    """dvs_mesh_components of a numpy index buffer uint32 [nt,3] -> (label uint32 [n_vertices]: the smallest vertex index of each
    vertex's component, n_bad: the triangles ignored for an index >= n_vertices)"""
    tdev = torch.device("cuda", device)
    n_vertices = int(n_vertices)
    tri, d_tri = _tri_to_device(tri, tdev)
    label = torch.empty(max(n_vertices, 1), dtype=torch.int32, device=tdev)
    bad = torch.zeros(1, dtype=torch.int32, device=tdev)
    with torch.cuda.device(tdev):
        check(lib.dvs_mesh_components(_stream_ptr(), n_vertices, d_tri.data_ptr(), len(tri), label.data_ptr(), bad.data_ptr()), "dvs_mesh_components")
        torch.cuda.synchronize()
    return label[:n_vertices].cpu().numpy().view(np.uint32), int(bad.cpu().numpy().view(np.uint32)[0])


def clean_mesh(xyz, rgb, tri, min_bp, normals=None, device=0):
    """dvs_mesh_clean_count / _write on numpy arrays: the components with fewer than min_bp / 10000 of the largest one's triangles are
    dropped (min_bp in 1/100 percent, 0..10000) -> (xyz, rgb, tri, normals or None, info) with info a dict of dvs_mesh_clean_info"""
    tdev = torch.device("cuda", device)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    nv = len(xyz)
    if len(rgb) != nv or (normals is not None and len(normals) != nv):
        raise DvsError("clean_mesh: xyz, rgb and normals differ in length")
    tri, d_tri = _tri_to_device(tri, tdev)

    def up(a, dtype):
        d = torch.empty((max(nv, 1), 3), dtype=dtype, device=tdev)
        if nv:
            d[:nv].copy_(torch.from_numpy(a))
        return d
    d_xyz, d_rgb = up(xyz, torch.float32), up(rgb, torch.uint8)
    d_nrm = None if normals is None else up(np.ascontiguousarray(normals, np.float32).reshape(-1, 3), torch.float32)
    scratch = torch.empty(lib.dvs_mesh_clean_scratch_bytes(nv, len(tri)) + 256, dtype=torch.uint8, device=tdev)
    sp = (scratch.data_ptr() + 255) & ~255
    info = MeshCleanInfo()
    with torch.cuda.device(tdev):
        check(lib.dvs_mesh_clean_count(_stream_ptr(), nv, d_tri.data_ptr(), len(tri), int(min_bp), sp, C.byref(info)), "dvs_mesh_clean_count")
        kv, kt = info.kept_vertices, info.kept_triangles
        o_xyz = torch.empty((max(kv, 1), 3), dtype=torch.float32, device=tdev)
        o_rgb = torch.empty((max(kv, 1), 3), dtype=torch.uint8, device=tdev)
        o_nrm = None if d_nrm is None else torch.empty((max(kv, 1), 3), dtype=torch.float32, device=tdev)
        o_tri = torch.empty((max(kt, 1), 3), dtype=torch.int32, device=tdev)
        check(lib.dvs_mesh_clean_write(_stream_ptr(), nv, d_xyz.data_ptr(), d_rgb.data_ptr(), None if d_nrm is None else d_nrm.data_ptr(), d_tri.data_ptr(),
                                       len(tri), sp, o_xyz.data_ptr(), o_rgb.data_ptr(), None if o_nrm is None else o_nrm.data_ptr(), o_tri.data_ptr()),
              "dvs_mesh_clean_write")
        torch.cuda.synchronize()
    return (o_xyz[:kv].cpu().numpy(), o_rgb[:kv].cpu().numpy(), o_tri[:kt].cpu().numpy().view(np.uint32),
            None if o_nrm is None else o_nrm[:kv].cpu().numpy(), {name: getattr(info, name) for name, _ in MeshCleanInfo._fields_})


def decimate_mesh(xyz, rgb, tri, origin, cell, ncell, normals=None, device=0):
    """dvs_mesh_decimate_count / _write on numpy arrays: vertex clustering on the lattice of ncell = (cx, cy, cz) cubic cells of edge
    `cell` from `origin` — every occupied cell's vertices become one vertex (mean position, colour, renormalised normal), collapsed and
    repeated triangles and unused clusters are dropped -> (xyz, rgb, tri, normals or None, info) with info a dict of dvs_mesh_decimate_info"""
    tdev = torch.device("cuda", device)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    nv = len(xyz)
    if len(rgb) != nv or (normals is not None and len(normals) != nv):
        raise DvsError("decimate_mesh: xyz, rgb and normals differ in length")
    tri, d_tri = _tri_to_device(tri, tdev)

    def up(a, dtype):
        d = torch.empty((max(nv, 1), 3), dtype=dtype, device=tdev)
        if nv:
            d[:nv].copy_(torch.from_numpy(a))
        return d
    d_xyz, d_rgb = up(xyz, torch.float32), up(rgb, torch.uint8)
    d_nrm = None if normals is None else up(np.ascontiguousarray(normals, np.float32).reshape(-1, 3), torch.float32)
    scratch = torch.empty(lib.dvs_mesh_decimate_scratch_bytes(nv, len(tri)) + 256, dtype=torch.uint8, device=tdev)
    sp = (scratch.data_ptr() + 255) & ~255
    info = MeshDecimateInfo()
    c_origin = (C.c_float * 3)(*[float(v) for v in origin])
    c_ncell = (C.c_int32 * 3)(*[int(v) for v in ncell])
    with torch.cuda.device(tdev):
        check(lib.dvs_mesh_decimate_count(_stream_ptr(), nv, d_xyz.data_ptr(), d_tri.data_ptr(), len(tri), c_origin, float(cell), c_ncell, sp,
                                          C.byref(info)), "dvs_mesh_decimate_count")
        ov, ot = info.out_vertices, info.out_triangles
        o_xyz = torch.empty((max(ov, 1), 3), dtype=torch.float32, device=tdev)
        o_rgb = torch.empty((max(ov, 1), 3), dtype=torch.uint8, device=tdev)
        o_nrm = None if d_nrm is None else torch.empty((max(ov, 1), 3), dtype=torch.float32, device=tdev)
        o_tri = torch.empty((max(ot, 1), 3), dtype=torch.int32, device=tdev)
        check(lib.dvs_mesh_decimate_write(_stream_ptr(), nv, d_xyz.data_ptr(), d_rgb.data_ptr(), None if d_nrm is None else d_nrm.data_ptr(),
                                          d_tri.data_ptr(), len(tri), sp, o_xyz.data_ptr(), o_rgb.data_ptr(),
                                          None if o_nrm is None else o_nrm.data_ptr(), o_tri.data_ptr()), "dvs_mesh_decimate_write")
        torch.cuda.synchronize()
    return (o_xyz[:ov].cpu().numpy(), o_rgb[:ov].cpu().numpy(), o_tri[:ot].cpu().numpy().view(np.uint32),
            None if o_nrm is None else o_nrm[:ov].cpu().numpy(), {name: getattr(info, name) for name, _ in MeshDecimateInfo._fields_})
