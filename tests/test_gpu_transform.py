"""dvs_transform_splats / dvs_transform_points (csrc/transform.hip) on the GPU against tests/transform_ref.py, bit for bit on every output
array: one lane, a partial tile, an exact tile, a tile plus a tail, several workgroups plus a tail; both shN layouts; degrees 0..3; in
place; guard bytes; refusals that launch nothing. And the end-to-end judge: a model and its camera moved together render the same picture."""
import ctypes as C
import numpy as np
import pytest
import transform_ref as T

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 1000, 2049)
ROWS, TILED = 0, 1
INVALID = 1
GUARD = 64
FILL = 0x5A
f32 = np.float32
KEYS = ("pos", "shN", "scale", "rot")


def _sim():
    from divshot_amd import transform as X
    sim = X.similarity_from_trs(*T.INVARIANCE_TRS)
    return sim, X.sh_rotation(sim.R)


def _model(n, seed=0):
    rng = np.random.default_rng(seed + n)
    return {"pos": (3 * rng.normal(size=(n, 3))).astype(f32), "shN": rng.normal(size=(n, 45)).astype(f32),
            "scale": (rng.normal(size=(n, 3)) - 2).astype(f32), "rot": rng.normal(size=(n, 4)).astype(f32)}


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _floats(n, layout):
    return {"pos": 3 * n, "shN": (n + 63) // 64 * 64 * 48 if layout == TILED else 45 * n, "scale": 3 * n, "rot": 4 * n}


def _guarded(dev, host):
    """a device buffer of FILL bytes with `host` (float32, flat) in its middle, 16-byte aligned; -> (buffer, payload pointer)"""
    import torch
    buf = torch.full((host.nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    buf[GUARD:GUARD + host.nbytes] = torch.from_numpy(host.view(np.uint8).copy()).to(dev)
    return buf, buf.data_ptr() + GUARD


def _payload(buf, nbytes):
    h = buf.cpu().numpy()
    assert (h[:GUARD] == FILL).all() and (h[GUARD + nbytes:] == FILL).all(), "a write outside the buffer"
    return h[GUARD:GUARD + nbytes].copy().view(f32)


def _run(dev, model, degree, layout, inplace=False, with_shn=True):
    """one dvs_transform_splats call -> dict of the output arrays as the device holds them (guards checked), and the return code"""
    import torch
    from divshot_amd._lib import lib
    sim, D = _sim()
    n = len(model["pos"])
    fl = _floats(n, layout)
    host = {k: np.ascontiguousarray(model[k], f32).reshape(-1) for k in KEYS}
    if layout == TILED:
        host["shN"] = T.tiled(model["shN"], pad=9.0)                            # the input's pads and dead lanes hold 9.0
    src = {k: _guarded(dev, host[k]) for k in KEYS}
    dst = src if inplace else {k: _guarded(dev, np.full(fl[k], np.frombuffer(bytes([FILL] * 4), f32)[0], f32)) for k in KEYS}
    shn_in, shn_out = (src["shN"][1], dst["shN"][1]) if with_shn else (None, None)
    rc = lib.dvs_transform_splats(_stream(), n, degree, C.byref(sim), D.ctypes.data, src["pos"][1], shn_in, layout, src["scale"][1], src["rot"][1],
                                  dst["pos"][1], shn_out, dst["scale"][1], dst["rot"][1])
    torch.cuda.synchronize()
    out = {k: _payload(dst[k][0], 4 * fl[k]) for k in KEYS}
    if not inplace:
        for k in KEYS:
            assert np.array_equal(_payload(src[k][0], 4 * fl[k]).view(np.uint32), host[k].view(np.uint32)), f"the input {k} was written"
    return rc, out


def _want(model, degree, layout):
    sim, D = _sim()
    w = T.transform_splats(sim.R, sim.t, sim.s, D, model["pos"], model["shN"], model["scale"], model["rot"], degree)
    w["shN"] = T.tiled(w["shN"]) if layout == TILED else w["shN"]             # pads and lanes past n: exactly 0
    return {k: np.ascontiguousarray(w[k], f32).reshape(-1) for k in KEYS}


@pytest.mark.parametrize("layout", [ROWS, TILED])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_restatement(gpu_device, n, layout):
    model = _model(n)
    for degree in range(4):
        rc, got = _run(gpu_device, model, degree, layout)
        assert rc == 0
        want = _want(model, degree, layout)
        for k in KEYS:
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (k, degree, int((got[k] != want[k]).sum()))
        rc, same = _run(gpu_device, model, degree, layout, inplace=True)
        assert rc == 0
        for k in KEYS:
            assert np.array_equal(same[k].view(np.uint32), got[k].view(np.uint32)), ("in place", k, degree)


def test_degree_zero_without_shn(gpu_device):
    model = _model(65)
    rc, got = _run(gpu_device, model, 0, TILED, with_shn=False)
    assert rc == 0
    want = _want(model, 0, TILED)
    for k in ("pos", "scale", "rot"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    assert (got["shN"].view(np.uint8) == FILL).all()                            # not touched


def test_invalid_arguments_launch_nothing(gpu_device):
    import torch
    from divshot_amd._lib import lib, Similarity
    sim, D = _sim()
    n = 100
    model = _model(n)
    host = {k: np.ascontiguousarray(model[k], f32).reshape(-1) for k in KEYS}
    host["shN"] = T.tiled(model["shN"])
    src = {k: _guarded(gpu_device, host[k]) for k in KEYS}
    dst = {k: _guarded(gpu_device, np.zeros_like(host[k])) for k in KEYS}
    for k in KEYS:
        dst[k][0].fill_(FILL)

    def call(n_=n, degree=3, sim_=sim, D_=D, layout=TILED, **ptr):
        a = {"pos": src["pos"][1], "shN": src["shN"][1], "scale": src["scale"][1], "rot": src["rot"][1], "pos_out": dst["pos"][1], "shN_out": dst["shN"][1],
             "scale_out": dst["scale"][1], "rot_out": dst["rot"][1]}
        a.update(ptr)
        return lib.dvs_transform_splats(_stream(), n_, degree, C.byref(sim_) if sim_ is not None else None, None if D_ is None else D_.ctypes.data, a["pos"],
                                        a["shN"], layout, a["scale"], a["rot"], a["pos_out"], a["shN_out"], a["scale_out"], a["rot_out"])

    bad_s, bad_R = Similarity.from_buffer_copy(sim), Similarity.from_buffer_copy(sim)
    bad_s.s = 0.0
    bad_R.R[0] = 2.0
    assert call(n_=0) == INVALID and call(n_=-5) == INVALID
    assert call(degree=-1) == INVALID and call(degree=4) == INVALID
    assert call(layout=2) == INVALID
    assert call(sim_=None) == INVALID and call(sim_=bad_s) == INVALID and call(sim_=bad_R) == INVALID and call(D_=None) == INVALID
    for name in ("pos", "scale", "rot", "pos_out", "scale_out", "rot_out", "shN", "shN_out"):
        assert call(**{name: None}) == INVALID, name
        assert call(**{name: src["pos"][1] + 4}) == INVALID, name                # off a 16-byte boundary
    torch.cuda.synchronize()
    for k in KEYS:
        assert (dst[k][0].cpu().numpy() == FILL).all(), k
    assert call() == 0


@pytest.mark.parametrize("n", (1, 255, 256, 257, 5000))
def test_points_equal_restatement(gpu_device, n):
    import torch
    from divshot_amd._lib import lib
    sim, _ = _sim()
    rng = np.random.default_rng(n)
    xyz, nrm = (4 * rng.normal(size=(n, 3))).astype(f32), rng.normal(size=(n, 3)).astype(f32)
    want_x, want_n = T.transform_points(sim.R, sim.t, sim.s, xyz, nrm)
    for with_normals in (True, False):
        sx, sn = _guarded(gpu_device, xyz.reshape(-1)), _guarded(gpu_device, nrm.reshape(-1))
        dx, dn = _guarded(gpu_device, np.zeros(3 * n, f32)), _guarded(gpu_device, np.zeros(3 * n, f32))
        dn[0].fill_(FILL)
        rc = lib.dvs_transform_points(_stream(), n, C.byref(sim), sx[1], sn[1] if with_normals else None, dx[1], dn[1] if with_normals else None)
        assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(_payload(dx[0], 12 * n).view(np.uint32), want_x.reshape(-1).view(np.uint32))
        if with_normals:
            assert np.array_equal(_payload(dn[0], 12 * n).view(np.uint32), want_n.reshape(-1).view(np.uint32))
        else:
            assert (dn[0].cpu().numpy() == FILL).all()
        rc = lib.dvs_transform_points(_stream(), n, C.byref(sim), sx[1], sn[1] if with_normals else None, sx[1], sn[1] if with_normals else None)     # in place
        assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(_payload(sx[0], 12 * n).view(np.uint32), want_x.reshape(-1).view(np.uint32))
        if with_normals:
            assert np.array_equal(_payload(sn[0], 12 * n).view(np.uint32), want_n.reshape(-1).view(np.uint32))
    assert lib.dvs_transform_points(_stream(), 0, C.byref(sim), sx[1], None, dx[1], None) == INVALID
    assert lib.dvs_transform_points(_stream(), n, C.byref(sim), None, None, dx[1], None) == INVALID
    assert lib.dvs_transform_points(_stream(), n, C.byref(sim), sx[1], sn[1], dx[1], None) == INVALID


def _camera(Rc, tc, size=64, fov=60.0):
    from divshot_amd._lib import lib, Camera
    cam = Camera()
    R, t = np.ascontiguousarray(Rc, f32).reshape(9), np.ascontiguousarray(tc, f32).reshape(3)
    assert lib.dvs_make_camera(R.ctypes.data, t.ctypes.data, C.c_float(fov), size, size, C.byref(cam)) == 0
    return cam


D_ORACLE = 2.801e-06


def test_render_invariance(gpu_device):
    """500 splats, 64x64, SH degree 3, depths in [2, 6]: (model, camera) and (T model, T camera) render the same picture through
    divshot_amd.raster, per pixel within d_oracle + 2e-4. d_oracle = 2.801e-06 is the largest difference between the fp32 CPU oracle's own
    two renders of the same two inputs (T model from the restatement), measured on the CPU for seed 3 of transform_ref.invariance_scene
    (seeds 1..8 give 6.1e-4, 1.9e-6, 2.8e-6, 2.3e-6, 2.1e-6, 1.6e-6, 1.8e-3, 1.9e-6: 1 and 7 carry a threshold flip); 2e-4 is twice the
    per-pixel HIP-vs-oracle bound of the parity suite. Control: with pos, scale, rot transformed and shN left unrotated some pixel must
    exceed the bar tenfold (the oracle's own figure for that: 1.07)."""
    import torch
    from divshot_amd import transform as X
    from divshot_amd.raster import Rasterizer, params_to_device
    model, Rc, cc = T.invariance_scene()
    n = len(model["opacity"])
    sim, D = _sim()
    r = Rasterizer(0, max_splats=1024, max_w=64, max_h=64)
    Pd = params_to_device(model, r.tdev)
    a = r.forward(Pd, _camera(Rc, -Rc @ cc), sh_degree=3).cpu().numpy().copy()
    pos, shN, scale, rot = X.transform_splats(sim, D, Pd["pos"], Pd["shN"].reshape(n, 45).contiguous(), Pd["scale"], Pd["rot"], 3, ROWS)
    moved = dict(Pd)
    moved.update(pos=pos, shN=shN.reshape(Pd["shN"].shape), scale=scale, rot=rot)
    cam2 = _camera(*T.moved_camera(sim.R, sim.t, sim.s, Rc, cc))
    b = r.forward(moved, cam2, sh_degree=3).cpu().numpy().copy()
    plain = dict(moved)
    plain["shN"] = Pd["shN"]
    c = r.forward(plain, cam2, sh_degree=3).cpu().numpy().copy()
    torch.cuda.synchronize()
    r.close()
    bar = D_ORACLE + 2e-4
    d, dc = np.abs(a - b).max(), np.abs(a - c).max()
    print(f"render invariance: max difference {d:.3e} (bar {bar:.3e}); shN left unrotated: {dc:.3e}")
    assert a.mean() > 0.1
    assert d <= bar
    assert dc >= 10 * bar
