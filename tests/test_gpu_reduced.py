"""dvs_sh_degree_select, dvs_codebooks_build, dvs_reduced_degree_counts, dvs_pack_reduced and dvs_unpack_reduced (csrc/reduced.hip) on
the GPU against tests/reduced_ply_ref.py. Centres, iteration counts, payloads and decoded arrays are compared with ==; the degrees with
== on every splat the float64 restatement decides by more than 1e-4 t + 1e-7 (at most 1 % are not, asserted before the device's answer
is looked at). Sizes: one lane, a partial tile, an exact tile, a tile plus a tail, several tiles; one and several scan tiles and sort
partitions for the codebooks."""
import ctypes as C
import numpy as np
import pytest
import reduced_ply_ref as R

pytestmark = pytest.mark.gpu

ROWS, TILED = 0, 1
INVALID = 1                                                  # DVS_ERR_INVALID
GUARD = 64
FILL = 0x5A
f32 = np.float32


def _tiled(shN, pad=0.0):
    shN = np.asarray(shN, f32).reshape(-1, 45)
    n = len(shN)
    tiles = (n + 63) // 64
    full = np.full((tiles * 64, 48), pad, f32)
    full[:n, :45] = shN
    return np.ascontiguousarray(full.reshape(tiles, 64, 12, 4).transpose(0, 2, 1, 3)).reshape(-1)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(dev, a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    assert t.data_ptr() % 16 == 0
    return t


def _guarded(dev, nbytes):
    import torch
    buf = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf


def _payload(buf, nbytes):
    h = buf.cpu().numpy()
    assert (h[:GUARD] == FILL).all() and (h[GUARD + nbytes:] == FILL).all(), "a write outside the buffer"
    return h[GUARD:GUARD + nbytes].copy()


def _upload(dev, model, layout):
    arrs = {k: np.ascontiguousarray(model[k], f32).reshape(-1) for k in R.FIELDS}
    if layout == TILED:
        arrs["shN"] = _tiled(model["shN"], pad=9.0)                          # (the pads are never read as values)
    return {k: _dev(dev, v) for k, v in arrs.items()}


def _scratch(dev, n):
    import torch
    from divshot_amd._lib import lib
    return torch.empty(lib.dvs_reduced_scratch_bytes(n), dtype=torch.uint8, device=dev)


def _build(dev, model, degrees, max_iters, layout=ROWS):
    import torch
    from divshot_amd._lib import lib
    n = len(degrees)
    src = _upload(dev, model, layout)
    deg = _dev(dev, np.asarray(degrees, np.uint8))
    centres = _guarded(dev, 4 * R.BOOKS * R.ENTRIES)
    iters = _guarded(dev, 4 * R.BOOKS)
    scratch = _scratch(dev, n)
    rc = lib.dvs_codebooks_build(_stream(), n, src["sh0"].data_ptr(), src["shN"].data_ptr(), layout, src["opacity"].data_ptr(),
                                 src["scale"].data_ptr(), src["rot"].data_ptr(), deg.data_ptr(), max_iters, scratch.data_ptr(),
                                 centres.data_ptr() + GUARD, iters.data_ptr() + GUARD)
    assert rc == 0
    torch.cuda.synchronize()
    return _payload(centres, 4 * R.BOOKS * R.ENTRIES).view(f32).reshape(R.BOOKS, R.ENTRIES), _payload(iters, 4 * R.BOOKS).view(np.int32)


# ---- codebooks ------------------------------------------------------------------------------------------------------------------------
def _values(kind, m, seed):
    r = np.random.default_rng(seed)
    if kind == "uniform":
        return r.uniform(-3, 3, m).astype(f32)
    if kind == "two_clusters":
        return np.where(r.random(m) < 0.5, r.uniform(-1.0, -0.999, m), r.uniform(7.0, 7.001, m)).astype(f32)
    if kind == "duplicates":                                                 # few distinct values, some of them tiny next to the largest
        pool = np.concatenate([r.uniform(-2, 2, 40), r.uniform(-1e-5, 1e-5, 10)]).astype(f32)
        return pool[r.integers(0, len(pool), m)]
    if kind == "mixed_sign":
        return (r.normal(0, 1, m) * r.choice([1e-3, 1.0, 50.0], m)).astype(f32)
    if kind == "all_equal":
        return np.full(m, f32(0.3337))
    if kind == "not_finite":
        v = r.uniform(-1, 1, m).astype(f32)
        v[::3] = np.nan
        v[1::7] = np.inf
        v[2::11] = -np.inf
        return v
    raise KeyError(kind)


def _model_with(values_n, values_3n):
    """a model whose opacity book (n values) and scale book (3 n values) are the given sets; the other arrays are tame"""
    n = len(values_n)
    m = R.random_model(n, seed=n)
    m["opacity"] = np.asarray(values_n, f32)
    m["scale"] = np.asarray(values_3n, f32).reshape(n, 3)
    return m


CODEBOOK_SIZES = (1, 255, 256, 257, 2047, 2048, 2049, 5000)                  # the scale book has 3 m values: up to 3 * 5000
KINDS = ("uniform", "two_clusters", "duplicates", "mixed_sign", "all_equal", "not_finite")


@pytest.mark.parametrize("max_iters", [1, 100])
@pytest.mark.parametrize("m", CODEBOOK_SIZES)
def test_codebooks_match_the_restatement(gpu_device, m, max_iters):
    """every kind of value set at every size: the opacity book carries the m values, the scale book 3 m of the next kind"""
    for k, kind in enumerate(KINDS):
        model = _model_with(_values(kind, m, 10 * m + k), _values(KINDS[(k + 1) % len(KINDS)], 3 * m, 20 * m + k))
        deg = R.degree_mix(m, "mixed", seed=m)
        with np.errstate(invalid="ignore", over="ignore"):
            want_c, want_i = R.build_codebooks(model, deg, max_iters)
        got_c, got_i = _build(gpu_device, model, deg, max_iters)
        print(f"m {m} {kind}: iterations {got_i.tolist()}")
        assert np.array_equal(got_i, want_i), (kind, got_i.tolist(), want_i.tolist())
        assert np.array_equal(got_c, want_c), (kind, np.argwhere(got_c != want_c)[:5].tolist())


@pytest.mark.parametrize("layout", [ROWS, TILED])
def test_rest_books_take_only_the_splats_that_store_the_coefficient(gpu_device, layout):
    """no splat above degree 1: the books of coefficients 3..14 are empty (all zero, 0 iterations), those of 0..2 hold a strict subset;
    the values of the splats that do not store a coefficient are huge, so a book that took them would show it"""
    n = 3000
    model = R.random_model(n, seed=9)
    deg = (np.arange(n) % 2).astype(np.uint8)
    model["shN"].reshape(n, 15, 3)[deg == 0] = 1e6
    model["shN"].reshape(n, 15, 3)[:, 3:] = -1e6
    want_c, want_i = R.build_codebooks(model, deg, 100)
    got_c, got_i = _build(gpu_device, model, deg, 100, layout)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_c, want_c)
    assert not got_c[4:16].any() and not got_i[4:16].any() and np.abs(got_c[1:4]).max() < 1 and got_i[1:4].min() >= 1
    a, b = _build(gpu_device, model, deg, 100, layout), _build(gpu_device, model, deg, 100, layout)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()            # two calls, identical bytes


# ---- pack / unpack --------------------------------------------------------------------------------------------------------------------
def _layout_of(counts, half):
    from divshot_amd._lib import lib, ReducedLayout
    L = ReducedLayout()
    assert lib.dvs_reduced_layout_for((C.c_uint32 * 4)(*[int(c) for c in counts]), int(half), C.byref(L)) == 0
    return L


def _counts(dev, degrees):
    import torch
    from divshot_amd._lib import lib
    n = len(degrees)
    deg = _dev(dev, np.asarray(degrees, np.uint8))
    out = _guarded(dev, 16)
    scratch = _scratch(dev, n)
    assert lib.dvs_reduced_degree_counts(_stream(), n, deg.data_ptr(), scratch.data_ptr(), out.data_ptr() + GUARD) == 0
    torch.cuda.synchronize()
    return _payload(out, 16).view(np.uint32)


def _pack(dev, model, degrees, centres, half, layout):
    import torch
    from divshot_amd._lib import lib
    n = len(degrees)
    counts = _counts(dev, degrees)
    assert counts.tolist() == np.bincount(np.minimum(degrees, 3), minlength=4).tolist()
    L = _layout_of(counts, half)
    src = _upload(dev, model, layout)
    deg = _dev(dev, np.asarray(degrees, np.uint8))
    cen = _dev(dev, np.asarray(centres, f32).reshape(-1))
    out = _guarded(dev, L.total)
    scratch = _scratch(dev, n)
    rc = lib.dvs_pack_reduced(_stream(), n, src["pos"].data_ptr(), src["sh0"].data_ptr(), src["shN"].data_ptr(), layout, src["opacity"].data_ptr(),
                              src["scale"].data_ptr(), src["rot"].data_ptr(), deg.data_ptr(), cen.data_ptr(), scratch.data_ptr(), C.byref(L),
                              out.data_ptr() + GUARD)
    assert rc == 0
    torch.cuda.synchronize()
    return _payload(out, L.total), L


def _unpack(dev, payload, L, n, layout):
    import torch
    from divshot_amd._lib import lib
    packed = _dev(dev, payload)
    shn_floats = (n + 63) // 64 * 64 * 48 if layout == TILED else n * 45
    floats = {"pos": 3 * n, "sh0": 3 * n, "shN": shn_floats, "opacity": n, "scale": 3 * n, "rot": 4 * n}
    out = {k: _guarded(dev, 4 * v) for k, v in floats.items()}
    degree = _guarded(dev, n)
    ptr = {k: out[k].data_ptr() + GUARD for k in out}
    rc = lib.dvs_unpack_reduced(_stream(), n, packed.data_ptr(), C.byref(L), ptr["pos"], ptr["sh0"], ptr["shN"], layout, ptr["opacity"], ptr["scale"],
                                ptr["rot"], degree.data_ptr() + GUARD)
    assert rc == 0
    torch.cuda.synchronize()
    got = {k: _payload(out[k], 4 * floats[k]).view(f32) for k in out}
    got["degree"] = _payload(degree, n)
    return got


@pytest.fixture(scope="module")
def reference():
    """model, degrees, the restatement's centres (5 iterations), payload and decoding, once per (n, mix, half)"""
    cache = {}

    def get(n, mix, half):
        if (n, mix) not in cache:
            m = R.random_model(n, seed=n)
            if n >= 65:                                                      # edge values: ids of NaN / inf, a degenerate quaternion, far positions
                m["opacity"][3], m["scale"][5, 1], m["sh0"][7, 2], m["shN"][9, 4] = np.nan, np.inf, -np.inf, np.nan
                m["rot"][11], m["rot"][12] = 0.0, (3e19, 3e19, 0, 0)
                m["pos"][13], m["pos"][14] = (70000.0, -70000.0, 65519.0), (np.nan, 1e-7, -6.1e-5)
            deg = R.degree_mix(n, mix, seed=n)
            with np.errstate(invalid="ignore", over="ignore"):
                centres, _ = R.build_codebooks(m, deg, 5)
            cache[(n, mix)] = (m, deg, centres)
        m, deg, centres = cache[(n, mix)]
        if (n, mix, half) not in cache:
            with np.errstate(invalid="ignore", over="ignore"):
                payload = R.pack(m, deg, centres, half)
            cache[(n, mix, half)] = (payload, R.decode(payload, np.bincount(deg, minlength=4), half))
        return (m, deg, centres) + cache[(n, mix, half)]
    return get


PACK_SIZES = (1, 63, 64, 65, 257, 5000)
MIXES = ("all0", "all3", "mixed", "no2")


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("layout", [ROWS, TILED])
@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("n", PACK_SIZES)
def test_pack_and_unpack_match_the_restatement(gpu_device, reference, n, mix, layout, half):
    """the payload byte for byte (the blocks' strides of 17 .. 68 bytes put the tiles' runs on and off 16-byte boundaries), then the
    decoder on that payload: every array, with the zeros above each splat's degree, the tiled pads and the lanes past n"""
    m, deg, centres, want, dec = reference(n, mix, half)
    got, L = _pack(gpu_device, m, deg, centres, half, layout)
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].ravel().tolist()
    out = _unpack(gpu_device, want, L, n, layout)
    assert np.array_equal(out["degree"], dec["degree"])
    for k in ("pos", "sh0", "opacity", "scale", "rot"):
        assert np.array_equal(out[k].view(np.uint32), dec[k].reshape(-1).view(np.uint32)), k
    shn = _tiled(dec["shN"]) if layout == TILED else dec["shN"].reshape(-1)
    assert np.array_equal(out["shN"].view(np.uint32), shn.view(np.uint32)), "shN"


def test_pack_is_deterministic_and_takes_out_of_order_centres(gpu_device):
    """two calls, identical bytes; centres that are not ascending (boundaries out of order) give the ids of the count rule"""
    n = 1000
    m = R.random_model(n, seed=77)
    deg = R.degree_mix(n, "mixed", seed=77)
    centres, _ = R.build_codebooks(m, deg, 3)
    centres[17][[20, 21, 22, 200]] = centres[17][[22, 20, 200, 21]]
    centres[3][[0, 255]] = centres[3][[255, 0]]
    want = R.pack(m, deg, centres, True)
    a, _ = _pack(gpu_device, m, deg, centres, True, TILED)
    b, _ = _pack(gpu_device, m, deg, centres, True, TILED)
    assert a.tobytes() == b.tobytes() and np.array_equal(a, want)


# ---- degree selection -----------------------------------------------------------------------------------------------------------------
def _select(dev, pos, shN, cams, D, t, layout):
    import torch
    from divshot_amd._lib import lib
    n = len(pos)
    p, c = _dev(dev, np.asarray(pos, f32).reshape(-1)), _dev(dev, np.asarray(cams, f32).reshape(-1))
    s = _dev(dev, _tiled(shN, pad=9.0) if layout == TILED else np.asarray(shN, f32).reshape(-1))
    out = _guarded(dev, n)
    assert lib.dvs_sh_degree_select(_stream(), n, D, p.data_ptr(), s.data_ptr(), layout, c.data_ptr(), len(cams), t, out.data_ptr() + GUARD) == 0
    torch.cuda.synchronize()
    return _payload(out, n)


@pytest.mark.parametrize("n,D,C", R.DEGREE_CASES)
def test_degree_selection_matches_the_restatement(gpu_device, n, D, C):
    t = 0.01
    pos, shN, cams = R.degree_case(n, D, C)
    want, undecided = R.select_degrees(pos, shN, cams, D, t)
    assert undecided.mean() <= 0.01 if n >= 65 else not undecided.any()      # from the restatement alone
    for layout in (ROWS, TILED):
        got = _select(gpu_device, pos, shN, cams, D, t, layout)
        print(f"n {n} D {D} C {C}: undecided {int(undecided.sum())}, histogram {np.bincount(got, minlength=4).tolist()}")
        assert np.array_equal(got[~undecided], want[~undecided]), np.argwhere(got != want)[:8].ravel().tolist()
        assert got.max() <= D


def test_degree_selection_not_finite_coefficients(gpu_device):
    """a NaN or infinite coefficient in band k keeps the splat at degree >= k; a camera at infinity is skipped"""
    pos, shN, cams = R.degree_case(200, 3, 7)
    shN = shN.copy().reshape(200, 15, 3)
    shN[:] = 0
    shN[0, 1, 0], shN[1, 5, 1], shN[2, 12, 2], shN[3, 9, 0] = np.nan, np.inf, -np.inf, np.nan
    cams[3] = (np.inf, 0, 0)
    want, undecided = R.select_degrees(pos, shN.reshape(200, 45), cams, 3, 0.01)
    assert want[:5].tolist() == [1, 2, 3, 3, 0] and not undecided.any()
    assert np.array_equal(_select(gpu_device, pos, shN.reshape(200, 45), cams, 3, 0.01, ROWS), want)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(gpu_device):
    import torch
    from divshot_amd._lib import lib
    n = 100
    m = R.random_model(n, seed=1)
    deg_h = R.degree_mix(n, "mixed", seed=1)
    src = _upload(gpu_device, m, ROWS)
    deg, cams = _dev(gpu_device, deg_h), _dev(gpu_device, np.ones(12, f32))
    scratch = _scratch(gpu_device, n)
    sentinel = lambda nbytes: torch.full((nbytes,), FILL, dtype=torch.uint8, device=gpu_device)
    out_deg, centres, iters, counts = sentinel(112), sentinel(4 * 20 * 256), sentinel(80), sentinel(16)
    L = _layout_of(np.bincount(deg_h, minlength=4), 0)
    payload = sentinel(L.total)
    dst = {k: sentinel(4 * src[k].numel()) for k in R.FIELDS}
    st = _stream()
    p = lambda t: t.data_ptr()

    sel = [n, 3, p(src["pos"]), p(src["shN"]), ROWS, p(cams), 4, 0.01, p(out_deg)]
    for k, bad in ((0, 0), (0, -3), (1, -1), (1, 4), (4, 2), (6, 0), (6, -1), (7, -0.5), (7, float("nan"))):
        args = list(sel)
        args[k] = bad
        assert lib.dvs_sh_degree_select(st, *args) == INVALID, (k, bad)
    for k in (2, 3, 5, 8):
        for bad in (None, sel[k] + 4):
            args = list(sel)
            args[k] = bad
            assert lib.dvs_sh_degree_select(st, *args) == INVALID, (k, bad)

    build = [n, p(src["sh0"]), p(src["shN"]), ROWS, p(src["opacity"]), p(src["scale"]), p(src["rot"]), p(deg), 100, p(scratch), p(centres), p(iters)]
    for k, bad in ((0, 0), (0, -1), (0, R.MAX_VALUES // 3 + 1), (3, 5), (8, 0)):      # (3 n above the cap: refused before anything is touched)
        args = list(build)
        args[k] = bad
        assert lib.dvs_codebooks_build(st, *args) == INVALID, (k, bad)
    for k in (1, 2, 4, 5, 6, 7, 9, 10, 11):
        for bad in (None, build[k] + 4):
            args = list(build)
            args[k] = bad
            assert lib.dvs_codebooks_build(st, *args) == INVALID, (k, bad)

    for args in ((0, p(deg), p(scratch), p(counts)), (n, None, p(scratch), p(counts)), (n, p(deg), None, p(counts)), (n, p(deg), p(scratch), None),
                 (n, p(deg), p(scratch), p(counts) + 4)):
        assert lib.dvs_reduced_degree_counts(st, *args) == INVALID

    pack = [n, p(src["pos"]), p(src["sh0"]), p(src["shN"]), ROWS, p(src["opacity"]), p(src["scale"]), p(src["rot"]), p(deg), p(centres), p(scratch),
            C.byref(L), p(payload)]
    unpack = [n, p(payload), C.byref(L), p(dst["pos"]), p(dst["sh0"]), p(dst["shN"]), ROWS, p(dst["opacity"]), p(dst["scale"]), p(dst["rot"]), None]
    other = _layout_of((n - 1, 1, 1, 0), 0)                                  # a layout of n + 1 splats
    broken = _layout_of(np.bincount(deg_h, minlength=4), 0)
    broken.off[2] += 1
    for fn, good, lay_at, shn_at in ((lib.dvs_pack_reduced, pack, 11, 4), (lib.dvs_unpack_reduced, unpack, 2, 6)):
        for k in range(len(good)):
            args = list(good)
            if k == 0:
                bads = (0, -1, n + 1)
            elif k == lay_at:
                bads = (None, C.byref(other), C.byref(broken))
            elif k == shn_at:
                bads = (-1, 2)
            elif good[k] is None:
                continue                                                     # (the nullable degree output)
            else:
                bads = (None, good[k] + 4)
            for bad in bads:
                args[k] = bad
                assert fn(st, *args) == INVALID, (fn.__name__, k)
    torch.cuda.synchronize()
    for t in (out_deg, centres, iters, counts, payload) + tuple(dst.values()):
        assert (t.cpu().numpy() == FILL).all()                               # nothing was launched
