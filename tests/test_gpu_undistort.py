"""dvs_undistort_view (csrc/undistort.hip) on the GPU against tests/undistort_ref.py: bytes, mask floats and the invalid count are all
defined bit for bit, so every comparison is ==. The smallest shapes that reach every path: 1x1, 17x1, 37x29 (odd width: byte and
float stores), 48x32 on aligned pointers (dword and 16-byte stores) and with dst 1 and 3 bytes off, 300x70 (two workgroups across, 18
down, the last one partial in both directions); planes 1, 3 and 4; with and without mask_src, mask_dst and invalid_count; a barrel, a
pincushion, a RADIAL camera with k1 and k2 of opposite sign, an OPENCV one with tangential terms, a principal point outside the
image, a camera that leaves every pixel invalid, and the identity. Every output sits between guard bytes; two calls return identical
results; invalid arguments are refused."""
import ctypes as C
import numpy as np
import pytest
import undistort_ref as U

pytestmark = pytest.mark.gpu

INVALID = 1
GUARD = 64
FILL = 0xA5
SHAPES = [(1, 1), (17, 1), (37, 29), (48, 32), (300, 70)]
CAMERAS = ["identity", "barrel", "pincushion", "radial", "opencv", "outside", "all_invalid"]


def camera(name, w, h):
    """-> (COLMAP model id, parameters)"""
    f = max(0.9 * w, 2.0)
    cx, cy = w / 2.0, h / 2.0
    return {"identity": (3, [f, 0.45 * w, 0.55 * h, 0.0, 0.0]),
            "barrel": (2, [f, cx, cy, -0.2]),
            "pincushion": (2, [f, cx, cy, 0.3]),
            "radial": (3, [f, cx + 0.75, cy - 0.5, 0.25, -0.1]),
            "opencv": (4, [f, 0.93 * f, 0.56 * w, 0.43 * h, 0.21, -0.06, 0.013, -0.009]),
            "outside": (4, [f, 1.1 * f, -0.3 * w, 1.4 * h, -0.05, 0.004, 0.002, 0.001]),
            "all_invalid": (2, [f, -5.0 * w - 3, -5.0 * h - 3, 5.0])}[name]


def inputs(w, h, planes=3, seed=0):
    r = np.random.default_rng(1000 * w + h + seed)
    return r.integers(0, 256, (planes, h, w), dtype=np.uint8), (r.random((h, w)) < 0.7).astype(np.uint8)


def ctypes_desc(desc):
    from divshot_amd._lib import UndistortDesc
    d = UndistortDesc()
    d.width, d.height = desc["width"], desc["height"]
    for n in U.FIELDS:
        setattr(d, n, float(desc[n]))
    return d


def run(dev, src, desc, mask_src=None, shift=0, with_mask=True, with_count=True, count_start=0):
    """-> (dst uint8 [planes][H][W], mask float32 [H][W] or None, count or None); dst starts `shift` bytes past a 16-byte boundary;
    dst and the mask sit between guard bytes that must come back untouched"""
    import torch
    from divshot_amd._lib import lib
    planes, h, w = src.shape
    n = planes * h * w
    d_src = torch.from_numpy(np.ascontiguousarray(src)).to(dev)
    d_msrc = torch.from_numpy(np.ascontiguousarray(mask_src)).to(dev) if mask_src is not None else None
    out = torch.full((n + 2 * GUARD + 16,), FILL, dtype=torch.uint8, device=dev)
    mout = torch.full((h * w * 4 + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    cnt = torch.full((3,), count_start, dtype=torch.int32, device=dev)           # the counter and a word on either side
    assert out.data_ptr() % 16 == 0 and mout.data_ptr() % 16 == 0
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    status = lib.dvs_undistort_view(st, C.byref(ctypes_desc(desc)), planes, d_src.data_ptr(), d_msrc.data_ptr() if d_msrc is not None else None,
                                    out.data_ptr() + GUARD + shift, mout.data_ptr() + GUARD if with_mask else None,
                                    cnt.data_ptr() + 4 if with_count else None)
    assert status == 0
    torch.cuda.synchronize()
    ho, hm, hc = out.cpu().numpy(), mout.cpu().numpy(), cnt.cpu().numpy()
    assert (ho[:GUARD + shift] == FILL).all() and (ho[GUARD + shift + n:] == FILL).all(), "a write outside dst"
    assert (hm[:GUARD] == FILL).all() and (hm[GUARD + 4 * h * w:] == FILL).all(), "a write outside mask_dst"
    assert hc[0] == count_start and hc[2] == count_start
    assert np.array_equal(d_src.cpu().numpy(), src), "the source was written"
    if not with_mask:
        assert (hm == FILL).all()
    if not with_count:
        assert hc[1] == count_start
    mask = hm[GUARD:GUARD + 4 * h * w].view(np.float32).reshape(h, w).copy() if with_mask else None
    return ho[GUARD + shift:GUARD + shift + n].reshape(planes, h, w).copy(), mask, int(hc[1]) - count_start if with_count else None


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), [got[tuple(b)].item() for b in bad[:5]], [want[tuple(b)].item() for b in bad[:5]])


@pytest.fixture(scope="module")
def reference():
    """reference(shape, camera name, planes, masked) -> (src, mask_src or None, desc, dst, mask, invalid), each computed once"""
    cache = {}

    def get(shape, name, planes=3, masked=True):
        key = (shape, name, planes, masked)
        if key not in cache:
            w, h = shape
            src, msrc = inputs(w, h, planes)
            desc = U.descriptor(*camera(name, w, h), w, h)
            cache[key] = (src, msrc if masked else None, desc) + U.undistort(src, desc, msrc if masked else None)
        return cache[key]
    return get


def test_the_cases_are_what_they_claim(reference):
    """on the reference alone, before the GPU is touched"""
    for shape in SHAPES:
        w, h = shape
        src, _, _, dst, mask, invalid = reference(shape, "identity", masked=False)
        assert np.array_equal(dst, src) and invalid == 0 and (mask == 1).all()
        assert reference(shape, "all_invalid")[5] == w * h and not reference(shape, "all_invalid")[3].any()
    for name in ("pincushion", "radial", "opencv", "outside"):
        invalid = reference((300, 70), name)[5]
        assert 0 < invalid < 300 * 70, name
    assert reference((300, 70), "barrel")[5] == 0
    _, _, _, _, with_src_mask, _ = reference((37, 29), "barrel")
    assert 0 < with_src_mask.sum() < reference((37, 29), "barrel", masked=False)[4].sum()


def test_pincushion_share_of_the_40x24_case():
    """the end-to-end capture's first camera (tests/test_gpu_dataset_undistort.py): the masked path is exercised and does not dominate"""
    _, _, invalid = U.undistort(np.zeros((1, 24, 40), np.uint8), U.descriptor(2, [36.0, 20.0, 12.0, 0.3], 40, 24))
    share = invalid / (40 * 24)
    print(f"invalid share of 40x24, f = 36, k1 = +0.3: {invalid} of 960 = {share:.4f}")
    assert 0.05 < share < 0.30


@pytest.mark.parametrize("name", CAMERAS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_bytes_mask_and_count_equal_the_restatement(gpu_device, reference, shape, name):
    src, msrc, desc, dst, mask, invalid = reference(shape, name)
    got, gmask, gcount = run(gpu_device, src, desc, msrc)
    same(got, dst, (shape, name, "bytes"))
    same(gmask, mask, (shape, name, "mask"))
    assert gcount == invalid


@pytest.mark.parametrize("shift", [1, 3])
def test_48x32_with_dst_off_the_dword_boundary(gpu_device, reference, shift):
    for name in ("pincushion", "opencv"):
        src, msrc, desc, dst, mask, invalid = reference((48, 32), name)
        got, gmask, gcount = run(gpu_device, src, desc, msrc, shift=shift)
        same(got, dst, (name, shift))
        same(gmask, mask, (name, shift))
        assert gcount == invalid


@pytest.mark.parametrize("planes", [1, 4])
@pytest.mark.parametrize("shape", [(37, 29), (48, 32)], ids=lambda s: "%dx%d" % s)
def test_one_and_four_planes(gpu_device, reference, shape, planes):
    src, msrc, desc, dst, mask, invalid = reference(shape, "opencv", planes)
    got, gmask, gcount = run(gpu_device, src, desc, msrc)
    same(got, dst, (shape, planes))
    same(gmask, mask, (shape, planes))
    assert gcount == invalid


@pytest.mark.parametrize("shape", [(37, 29), (48, 32)], ids=lambda s: "%dx%d" % s)
def test_every_optional_pointer_may_be_null(gpu_device, reference, shape):
    src, msrc, desc, dst, mask, invalid = reference(shape, "pincushion")
    _, _, _, _, validity, _ = reference(shape, "pincushion", masked=False)
    for with_src, with_mask, with_count in [(False, True, True), (True, False, True), (True, True, False), (False, False, False)]:
        got, gmask, gcount = run(gpu_device, src, desc, msrc if with_src else None, with_mask=with_mask, with_count=with_count, count_start=7)
        same(got, dst, (with_src, with_mask, with_count))
        if with_mask:
            same(gmask, mask if with_src else validity, "mask")                  # without a source mask the output mask is the validity
        if with_count:
            assert gcount == invalid                                             # the counter is incremented, not set: it started at 7


def test_the_golden_case(gpu_device):
    g = np.load(U.GOLDEN)
    desc = dict(width=37, height=29, **{n: g["desc"][k] for k, n in enumerate(U.FIELDS)})
    got, gmask, gcount = run(gpu_device, g["src"], desc)
    same(got, g["dst"], "golden bytes")
    same(gmask, g["mask"], "golden mask")
    assert gcount == int(g["invalid"])
    _, gmask, _ = run(gpu_device, g["src"], desc, g["src_mask"])
    same(gmask, g["mask_with_source_mask"], "golden mask with a source mask")


def test_two_calls_identical_results(gpu_device, reference):
    src, msrc, desc = reference((300, 70), "opencv")[:3]
    a, b = run(gpu_device, src, desc, msrc), run(gpu_device, src, desc, msrc)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def test_the_python_wrapper(gpu_device, reference):
    import torch
    from divshot_amd import _lib, train_ops
    src, msrc, _, _, _, _ = reference((48, 32), "opencv")
    model, params = camera("opencv", 48, 32)
    d = _lib.undistort_desc(model, params, 48, 32)
    dst, mask, invalid = U.undistort(src, U.descriptor(model, params, 48, 32), msrc)
    got, gmask, gcount = train_ops.undistort_view(torch.from_numpy(src).to(gpu_device), d, torch.from_numpy(msrc).to(gpu_device))
    same(got.cpu().numpy(), dst, "wrapper bytes")
    same(gmask.cpu().numpy(), mask, "wrapper mask")
    assert int(gcount.item()) == invalid
    got, gmask, _ = train_ops.undistort_view(torch.from_numpy(src).to(gpu_device), d)
    same(gmask.cpu().numpy(), U.undistort(src, U.descriptor(model, params, 48, 32))[1], "wrapper validity")
    with pytest.raises(ValueError):
        train_ops.undistort_view(torch.from_numpy(src[:, :-1]).contiguous().to(gpu_device), d)


def test_invalid_arguments(gpu_device):
    import torch
    from divshot_amd._lib import lib
    w, h = 40, 24
    desc = ctypes_desc(U.descriptor(2, [36.0, 20.0, 12.0, 0.3], w, h))
    src = torch.zeros(4 * w * h, dtype=torch.uint8, device=gpu_device)
    dst = torch.zeros(4 * w * h, dtype=torch.uint8, device=gpu_device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(d=desc, planes=3, s=src.data_ptr(), q=dst.data_ptr()):
        return lib.dvs_undistort_view(st, C.byref(d) if d is not None else None, planes, s, None, q, None, None)
    assert call() == 0
    assert call(d=None) == INVALID and call(s=None) == INVALID and call(q=None) == INVALID
    assert call(planes=0) == INVALID and call(planes=5) == INVALID and call(planes=-1) == INVALID
    assert call(q=src.data_ptr()) == INVALID                                     # dst == src
    assert call(q=src.data_ptr() + 3 * w * h - 1) == INVALID and call(s=dst.data_ptr() + 1, planes=1) == INVALID      # partial overlaps
    assert call(planes=1, q=src.data_ptr() + w * h) == 0                         # adjacent, not overlapping
    for field, value in (("width", 0), ("height", 0), ("width", -4), ("width", 65537), ("height", 65537)):
        d = ctypes_desc(U.descriptor(2, [36.0, 20.0, 12.0, 0.3], w, h))
        setattr(d, field, value)
        assert call(d=d) == INVALID, (field, value)
    torch.cuda.synchronize()
