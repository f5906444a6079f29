"""The scene of the replay-pass tests (test_gpu_depth.py, test_gpu_importance.py, test_gpu_sky.py) and the export of the forward state they
hand to their references. Two views of 50x37 (4x3 tiles, neither size a multiple of 16), 700 splats: 370 small ones spread over pixels
x < 40, y < 28 (tile (3, 2) stays empty), 300 faint ones crowded into tile (1, 0) and a stack of 30 opaque ones over pixel (10, 20)."""
import ctypes as C
import numpy as np
import divshot_amd as dv
from divshot_amd import _lib

W, H, N = 50, 37, 700


def cameras():
    cams = []
    for tx in (0.0, 0.08):
        cam = dv.Camera()
        R = np.eye(3, dtype=np.float32); t = np.array([tx, -0.02 * (tx > 0), 0.0], np.float32)
        _lib.check(dv.lib.dvs_make_camera(R.ctypes.data, t.ctypes.data, 60.0, W, H, C.byref(cam)), "dvs_make_camera")
        cams.append(cam)
    return cams


def scene_params(seed):
    r = np.random.default_rng(seed)
    fx = W / (2 * np.tan(np.radians(30.0))); fy = fx            # (tan_fovy = tan_fovx H / W)
    px = np.concatenate([r.uniform(2, 38, 370), r.uniform(20, 27, 300), 10 + r.normal(0, 0.4, 30)])
    py = np.concatenate([r.uniform(2, 26, 370), r.uniform(4, 11, 300), 20 + r.normal(0, 0.4, 30)])
    z = np.concatenate([r.uniform(3, 6, 370), r.uniform(3, 6, 300), np.linspace(2.5, 5.5, 30)])
    pos = np.stack([(px - (W - 1) / 2) * z / fx, (py - (H - 1) / 2) * z / fy, z], 1)
    sig = np.concatenate([r.uniform(0.06, 0.14, 370), r.uniform(0.08, 0.16, 300), np.full(30, 0.3)])
    P = {"pos": pos, "sh0": r.normal(0, 1, (N, 3)), "shN": np.zeros((N, 15, 3)),
         "opacity": np.concatenate([r.normal(0, 1.5, 370), r.normal(-3.4, 0.2, 300), np.full(30, 5.0)]),
         "scale": np.log(sig)[:, None] + r.normal(0, 0.15, (N, 3)), "rot": r.normal(0, 1, (N, 4))}
    return {k: np.ascontiguousarray(v, np.float32) for k, v in P.items()}


def export_view(r, v, V):
    st = _lib.FwdState()
    _lib.check(dv.lib.dvs_get_view_state(r.ctx, v, C.byref(st)), "dvs_get_view_state")
    st0 = _lib.FwdState()
    _lib.check(dv.lib.dvs_get_view_state(r.ctx, 0, C.byref(st0)), "dvs_get_view_state")
    tiles, hw = st.tiles_x * st.tiles_y, (st.height, st.width)       # (the view's own size: tests/test_gpu_list_seams.py exports other scenes)
    return dict(splat2d=r._d2h(st0.splat2d, (V * st.n, 16), np.float32), ranges=r._d2h(st.ranges, (tiles, 2), np.uint32),
                sorted_splat=r._d2h(st0.sorted_splat, (int(r.num_rendered),), np.uint32), n_contrib=r._d2h(st.n_contrib, hw, np.uint32),
                final_T=r._d2h(st.final_T, hw, np.float32))
