"""Surface extraction — Python handles over include/dvs_mesh.h and dvs_raster_depth_views (include/dvs_raster.h).

torch supplies device buffers and the HIP stream; all compute runs in libdvsraster.so:
    depth, alpha = depth_maps(rasterizer)              # of the rasterizer's last forward / forward_views
    grid = TsdfGrid((x0, y0, z0), voxel, (nx, ny, nz)); grid.integrate(cams, depth, alpha, rgb, trunc=4 * voxel)
    xyz, rgb, tri = grid.extract()                      # numpy: float32 [nv,3], uint8 [nv,3], uint32 [nt,3]
"""
import ctypes as C
import numpy as np
import torch
from ._lib import lib, Camera, Opts, TsdfGridDesc, check, DvsError, write_mesh_ply  # noqa: F401
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

    def extract(self):
        """marching tetrahedra over the grid -> (xyz float32 [nv,3], rgb uint8 [nv,3], tri uint32 [nt,3]) as numpy"""
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
            torch.cuda.synchronize()
        return xyz[:nv.value].cpu().numpy(), rgb[:nv.value].cpu().numpy(), tri[:nt.value].cpu().numpy().view(np.uint32)
