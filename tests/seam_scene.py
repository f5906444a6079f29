"""Scenes whose tile lists end where the list walks can go wrong (tests/test_seam_scene.py pins them on the CPU oracle,
tests/test_gpu_list_seams.py runs the kernels on them). Every walk stages a tile's list through LDS in batches of 256 entries and the
composite forward works in 64-entry words inside a batch; these scenes put the end of a list, and the end of a pixel's walk, on and
next to those seams. Plain numpy; three views each, so a batch launch has 3 or 18 tiles and workgroups without a tile.

len<L> (L in LENGTHS): 16x16, one tile per view. L broad faint splats with centres inside the image and distinct depths: the view's list
    has exactly L entries. sigma is 2.5 to 4 pixels and the opacity 0.006 to 0.016, so alpha = opacity G crosses 1/255 inside the tile:
    every entry is taken by the pixels near its centre and skipped by the others, and no pixel's T falls below 1e-3 — n_contrib
    reaches the last entries. The three cameras differ by a fraction of a pixel.
stop256, stop257: the 513-entry scene with three opaque tile-covering splats at depth ranks p, p + 1, p + 2 (1-based list positions).
    alpha is capped at 0.99: the entry at p takes T to 0.01 T, the entry at p + 1 would take it under 1e-4, so the forward ends every
    pixel there and n_contrib = p. p = 256: the walk ends with the first batch, the forward breaks at the top of the second.
tiles: 48x32 (3x2 tiles), 700 splats. View 1 looks away and sees nothing. In views 0 and 2 tile (2, 1) is empty, 560 faint splats crowd
    tile (0, 0) (a list of more than 512), 110 small ones give the other tiles short lists, and 30 opaque ones stacked over pixel
    (8, 24) saturate it. Splats spill between tiles; the lengths are whatever the binning gives.

SEEDS: chosen in tests/test_seam_scene.py's terms — for each scene the first seed from 1 for which, in all three views, the references
(depth_ref, importance_ref, sky_ref on the fp32 oracle's state) leave out no more than the caps allow. A faint scene has about
200 000 (pixel, entry) pairs per view with alpha spread over a factor of a few around 1/255, and one pair inside the references' 1e-5
band puts every splat behind it in doubt, so a seed passes only if no pair of the first 99 % of a list falls into the band."""
import ctypes as C
import numpy as np
import divshot_amd as dv
from divshot_amd import _lib

LENGTHS = (63, 64, 65, 255, 256, 257, 511, 512, 513, 769)
STOPS = (256, 257)
NAMES = tuple(f"len{L}" for L in LENGTHS) + tuple(f"stop{p}" for p in STOPS) + ("tiles",)
SEEDS = {"len63": 1, "len64": 1, "len65": 1, "len255": 2, "len256": 3, "len257": 2, "len511": 12, "len512": 1, "len513": 3, "len769": 39,
         "stop256": 3, "stop257": 3, "tiles": 1}
V = 3
FOV = 60.0
BG = (0.25, 0.5, 0.75)


def _camera(R, t, W, H, bg):
    cam = dv.Camera()
    R = np.ascontiguousarray(R, np.float32); t = np.ascontiguousarray(t, np.float32)
    _lib.check(dv.lib.dvs_make_camera(R.ctypes.data, t.ctypes.data, FOV, W, H, C.byref(cam)), "dvs_make_camera")
    cam.bg[0], cam.bg[1], cam.bg[2] = bg
    return cam


def _focal(W):
    return W / (2 * np.tan(np.radians(FOV / 2)))


def _pack(px, py, z, sig_px, opacity, r, W, H, iso=None):
    """centres in pixels, depths, sigmas in pixels, opacities in (0, 1) -> the parameter arrays (logit opacity, log scale)"""
    n = px.size
    f = _focal(W)
    pos = np.stack([(px - (W - 1) / 2) * z / f, (py - (H - 1) / 2) * z / f, z], 1)
    scale = np.log(sig_px * z / f)[:, None] + r.normal(0, 0.1, (n, 3))
    rot = r.normal(0, 1, (n, 4))
    shN = np.zeros((n, 15, 3)); shN[:, :3] = r.normal(0, 0.3, (n, 3, 3))
    sh0 = r.normal(0, 1, (n, 3))
    if iso is not None:                                           # the opaque covers: round, so the footprint is what sig_px says
        scale[iso] = np.log(sig_px[iso] * z[iso] / f)[:, None]; rot[iso] = [1.0, 0, 0, 0]
    P = {"pos": pos, "sh0": sh0, "shN": shN, "opacity": np.log(opacity / (1 - opacity)), "scale": scale, "rot": rot}
    return {k: np.ascontiguousarray(v, np.float32) for k, v in P.items()}


def single_tile(L, seed, stop=None):
    """-> (params, W, H); stop: None or the 1-based list position every pixel's walk ends at"""
    W = H = 16
    r = np.random.default_rng(seed)
    px, py = r.uniform(1.5, 13.5, L), r.uniform(1.5, 13.5, L)
    rank = r.permutation(L)                                        # the splat's position in the depth order
    z = 3.0 + 3.0 * rank / max(L - 1, 1)
    sig = r.uniform(2.5, 4.0, L)
    op = r.uniform(0.006, 0.016, L)
    iso = None
    if stop is not None:
        iso = np.flatnonzero((rank >= stop - 1) & (rank <= stop + 1))
        px[iso] = py[iso] = 7.5; sig[iso] = 150.0; op[iso] = 1.0 - 1e-5
    return _pack(px, py, z, sig, op, r, W, H, iso), W, H


def single_tile_cameras(bg=BG):
    shifts = ((0.0, 0.0), (0.1, -0.05), (-0.07, 0.08))            # at depth 3 to 6 and a focal length of 13.9 pixels: under half a pixel
    return [_camera(np.eye(3), (tx, ty, 0.0), 16, 16, bg) for tx, ty in shifts]


N_CROWD, N_TOP, N_BOTTOM, N_STACK = 560, 60, 50, 30


def tiles(seed):
    W, H = 48, 32
    r = np.random.default_rng(seed)
    cat = np.concatenate
    px = cat([r.uniform(3, 12, N_CROWD), r.uniform(2, 45, N_TOP), r.uniform(2, 26, N_BOTTOM), 8 + r.normal(0, 0.4, N_STACK)])
    py = cat([r.uniform(3, 12, N_CROWD), r.uniform(2, 9, N_TOP), r.uniform(20, 29, N_BOTTOM), 24 + r.normal(0, 0.4, N_STACK)])
    z = cat([r.uniform(3, 6, N_CROWD + N_TOP + N_BOTTOM), np.linspace(2.5, 5.5, N_STACK)])
    sig = cat([r.uniform(1.0, 1.8, N_CROWD), r.uniform(0.5, 1.2, N_TOP + N_BOTTOM), np.full(N_STACK, 2.0)])
    logit = cat([r.normal(-3.4, 0.2, N_CROWD), r.normal(0, 1.5, N_TOP + N_BOTTOM), np.full(N_STACK, 5.0)])
    return _pack(px, py, z, sig, 1 / (1 + np.exp(-logit)), r, W, H), W, H


def tiles_cameras(bg=BG):
    away = np.diag([-1.0, 1.0, -1.0])                              # half a turn about the vertical axis: every splat is behind it
    return [_camera(np.eye(3), (0.0, 0.0, 0.0), 48, 32, bg), _camera(away, (0.0, 0.0, 0.0), 48, 32, bg), _camera(np.eye(3), (0.06, -0.03, 0.0), 48, 32, bg)]


def scene(name, seed=None, bg=BG):
    """-> dict(name, P, cams, W, H, n, length: the requested list length or None, stop: the requested last contributor or None)"""
    seed = SEEDS[name] if seed is None else seed
    if name == "tiles":
        P, W, H = tiles(seed)
        return dict(name=name, P=P, cams=tiles_cameras(bg), W=W, H=H, n=P["pos"].shape[0], length=None, stop=None)
    stop = int(name[4:]) if name.startswith("stop") else None
    L = 513 if stop else int(name[3:])
    P, W, H = single_tile(L, seed, stop)
    return dict(name=name, P=P, cams=single_tile_cameras(bg), W=W, H=H, n=L, length=L, stop=stop)


def colourless(P):
    """every splat's colour clamped to zero, as tests/test_gpu_sky.py makes its scenes: the composite backward then leaves the geometry
    columns of the rows to the sky pass"""
    P = {k: v.copy() for k, v in P.items()}
    P["sh0"][:] = -10.0; P["shN"][:] = 0.0
    return P


def tile_lengths(ranges):
    ranges = np.asarray(ranges, np.int64)
    return ranges[:, 1] - ranges[:, 0]


def per_pixel_length(ranges, W, H):
    """the length of the list each pixel walks, [H,W]"""
    tx = (W + 15) // 16
    return tile_lengths(ranges)[(np.arange(H)[:, None] // 16) * tx + np.arange(W)[None, :] // 16]


def check_cases(sc, views):
    """what a scene claims, asserted from a forward's own state: views = one dict(ranges, n_contrib, final_T) per view, the CPU oracle's
    or the device's. Returns per view (list lengths, largest n_contrib) for the caller to print."""
    W, H, out = sc["W"], sc["H"], []
    assert len(views) == V
    for v, e in enumerate(views):
        length, nc, T = tile_lengths(e["ranges"]), np.asarray(e["n_contrib"], np.int64), np.asarray(e["final_T"], np.float64)
        assert nc.shape == (H, W) and (nc <= per_pixel_length(e["ranges"], W, H)).all()
        out.append((length.tolist(), int(nc.max())))
        if sc["name"] == "tiles":
            if v == 1:
                assert (length == 0).all() and (nc == 0).all() and (T == 1).all(), "the middle view sees something"
                continue
            assert length.size == 6 and length[5] == 0, ("tile (2, 1) is not empty", length)
            assert length.max() > 512 and nc.max() > 512, (length, nc.max())
            assert ((length > 0) & (length < 256)).sum() >= 3, ("no short lists", length)
            sat = T < 1e-2
            assert sat.any() and (nc[sat] < per_pixel_length(e["ranges"], W, H)[sat]).any(), "no saturated pixel that stops short of its list"
        elif sc["stop"]:
            assert length.tolist() == [sc["length"]], length
            assert nc.max() == sc["stop"] and (nc == sc["stop"]).mean() >= 0.5, (nc.max(), (nc == sc["stop"]).mean())
        else:
            assert length.tolist() == [sc["length"]], length
            assert T.min() > 1e-3, T.min()
            assert nc.max() > sc["length"] - 64, nc.max()
    return out
