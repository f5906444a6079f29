"""dvs_knn_mean_dist2 / dvs_init_from_points (csrc/knn.hip) on the GPU against tests/knn_ref.py. dist2 is compared bit for bit: the box
pruning of the search may not change a single value. Sizes: 1-4 (fewer than three neighbours), one short of / exactly / one past a
wavefront (64) and a box (1024), 5000 (several boxes, a partial last one); at 20 000 a uniform cloud, 20 tight clusters far apart
(pruning decides), all points on one line (zero extent on two Morton axes) and a 27^3 lattice with 317 exact duplicates (mass ties,
zero distances).

The bound on scale. scale = 0.5f * logf(max(dist2, 1e-7f)) with the device's logf. No accuracy table of the device's math functions
is installed with this ROCm tree, so the bound is the one its device library (ocml) is built to: the OpenCL full-profile limit for
log, 3 ulp (OpenCL C specification, "Relative error as ULPs"; HIP's published table of measured errors lists 1 for logf). Halving is
exact, so 3 ulp of the logarithm are 3 ulp of the scale; one more ulp for the multiply as the issue words it: |scale - ref| <= 4 ulp
of the float32 value of ref = 0.5 log(max(dist2, 1e-7)) in float64."""
import ctypes as C
import numpy as np
import pytest
import knn_ref as K

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 4, 63, 64, 65, 1023, 1024, 1025, 5000)
BIG = {"uniform": lambda: K.uniform(20000, 7), "clusters": lambda: K.clusters(20000, 8), "line": lambda: K.line(20000, 9),
       "lattice_with_duplicates": lambda: K.lattice(10)}
INVALID = 1                                                  # DVS_ERR_INVALID
GUARD = 16                                                   # 32-bit words kept around every output (64 B: the outputs stay 16-byte aligned)
FILL = 0x5A5A5A5A
SCALE_ULPS = 4


def _guarded(dev, words):
    import torch
    buf = torch.full((words + 2 * GUARD,), FILL, dtype=torch.int32, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf


def _payload(buf, words):
    h = buf.cpu().numpy().view(np.uint32)
    assert (h[:GUARD] == FILL).all() and (h[GUARD + words:] == FILL).all(), "a write outside the output"
    return h[GUARD:GUARD + words].copy()


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _knn(dev, pos):
    import torch
    from divshot_amd._lib import lib
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    n = len(pos)
    d_pos = torch.from_numpy(pos.reshape(-1)).to(dev)
    scratch = torch.empty(lib.dvs_knn_scratch_bytes(n), dtype=torch.uint8, device=dev)
    out = _guarded(dev, n)
    assert lib.dvs_knn_mean_dist2(_stream(), n, d_pos.data_ptr(), scratch.data_ptr(), out.data_ptr() + 4 * GUARD) == 0
    torch.cuda.synchronize()
    return _payload(out, n).view(np.float32)


def _assert_same(got, want, what):
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.fixture(scope="module")
def big_reference():
    """the 20 000-point inputs and their all-pairs results, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            pos = BIG[name]()
            cache[name] = (pos, K.mean_dist2(pos))
        return cache[name]
    return get


@pytest.mark.parametrize("n", SIZES)
def test_dist2_bit_for_bit_small(gpu_device, n):
    pos = K.uniform(n, 100 + n)
    got, want = _knn(gpu_device, pos), K.mean_dist2(pos)
    _assert_same(got, want, n)
    if n == 1:
        assert got[0] == 0.0
    if n == 2:
        d = pos[1] - pos[0]
        assert got[0] == got[1] == (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


@pytest.mark.parametrize("name", list(BIG))
def test_dist2_bit_for_bit_20000(gpu_device, big_reference, name):
    pos, want = big_reference(name)
    assert len(pos) == 20000
    got = _knn(gpu_device, pos)
    _assert_same(got, want, name)
    if name == "lattice_with_duplicates":
        assert (want < np.float32(0.25)).sum() >= 317                        # a duplicated point: (0 + 0.25 + 0.25) / 3 or less
    if name == "line":
        assert (got > 0).all()


def test_two_calls_identical_bytes(gpu_device, big_reference):
    pos, _ = big_reference("clusters")
    assert _knn(gpu_device, pos).tobytes() == _knn(gpu_device, pos).tobytes()


def test_init_from_points(gpu_device):
    import torch
    from divshot_amd._lib import lib
    n = 1500
    r = np.random.default_rng(4)
    rgb = r.integers(0, 256, (n, 3), dtype=np.uint8)
    rgb[0], rgb[1] = (0, 0, 0), (255, 255, 255)
    dist2 = np.exp(r.uniform(-20.0, 5.0, n)).astype(np.float32)
    dist2[:4] = (0.0, 1e-7, 5e-8, 1.0)
    pos = r.normal(size=(n, 3)).astype(np.float32)
    d_pos, d_d2 = torch.from_numpy(pos.reshape(-1)).to(gpu_device), torch.from_numpy(dist2).to(gpu_device)
    d_rgb = torch.from_numpy(rgb.reshape(-1)).to(gpu_device)
    outs = [_guarded(gpu_device, w) for w in (3 * n, n, 3 * n, 4 * n)]
    rc = lib.dvs_init_from_points(_stream(), n, d_pos.data_ptr(), d_rgb.data_ptr(), d_d2.data_ptr(), *[o.data_ptr() + 4 * GUARD for o in outs])
    assert rc == 0
    torch.cuda.synchronize()
    sh0, opacity, scale, rot = [_payload(o, w).view(np.float32) for o, w in zip(outs, (3 * n, n, 3 * n, 4 * n))]
    f = np.float32
    want_sh0 = (rgb.astype(f) / f(255.0) - f(0.5)) / f(0.28209479177387814)
    assert want_sh0.dtype == f and np.array_equal(sh0.view(np.uint32), want_sh0.reshape(-1).view(np.uint32))
    want_opa = f(np.log(np.float64(f(0.1) / f(0.9))))                        # logf(0.1f / 0.9f), correctly rounded
    assert np.array_equal(opacity.view(np.uint32), np.full(n, want_opa, f).view(np.uint32))
    assert np.array_equal(rot.reshape(n, 4), np.tile(np.array([1, 0, 0, 0], f), (n, 1)))
    scale = scale.reshape(n, 3)
    assert np.array_equal(scale[:, 0], scale[:, 1]) and np.array_equal(scale[:, 0], scale[:, 2])
    ref = 0.5 * np.log(np.maximum(dist2, f(1e-7)).astype(np.float64))
    ulps = np.abs(scale[:, 0].astype(np.float64) - ref) / np.spacing(np.abs(ref).astype(f)).astype(np.float64)
    print(f"scale: worst {ulps.max():.3f} ulp of 0.5 log(dist2)")
    assert ulps.max() <= SCALE_ULPS
    floor = 0.5 * np.log(np.float64(f(1e-7)))
    for k in (0, 2):                                                         # dist2 = 0 and dist2 < 1e-7 give 0.5 log(1e-7)
        assert scale[k, 0] == scale[1, 0] and abs(float(scale[k, 0]) - floor) <= SCALE_ULPS * float(np.spacing(f(abs(floor))))


def test_invalid_arguments(gpu_device):
    import torch
    from divshot_amd._lib import lib
    n = 300
    pos = torch.from_numpy(K.uniform(n, 1).reshape(-1)).to(gpu_device)
    scratch = torch.empty(lib.dvs_knn_scratch_bytes(n), dtype=torch.uint8, device=gpu_device)
    out = torch.zeros(16 * n + 64, dtype=torch.float32, device=gpu_device)
    rgb = torch.zeros(3 * n + 64, dtype=torch.uint8, device=gpu_device)
    st = _stream()
    assert lib.dvs_knn_scratch_bytes(0) == 0 and lib.dvs_knn_scratch_bytes(-5) == 0 and lib.dvs_knn_scratch_bytes(n) % 16 == 0
    good = [pos.data_ptr(), scratch.data_ptr(), out.data_ptr()]
    assert lib.dvs_knn_mean_dist2(st, n, *good) == 0
    for bad_n in (0, -1):
        assert lib.dvs_knn_mean_dist2(st, bad_n, *good) == INVALID
    for i in range(3):
        args = list(good)
        args[i] = good[i] + 4                                                # off a 16-byte boundary
        assert lib.dvs_knn_mean_dist2(st, n, *args) == INVALID, i
        args[i] = None
        assert lib.dvs_knn_mean_dist2(st, n, *args) == INVALID, i
    base = out.data_ptr()
    good = [pos.data_ptr(), rgb.data_ptr(), base, base + 4096, base + 4096 + 16 * n, base + 4096 + 32 * n, base + 4096 + 48 * n]
    assert all(p % 16 == 0 for p in good)
    assert lib.dvs_init_from_points(st, n, *good) == 0
    for bad_n in (0, -1):
        assert lib.dvs_init_from_points(st, bad_n, *good) == INVALID
    for i in range(len(good)):
        args = list(good)
        args[i] = good[i] + 4
        assert lib.dvs_init_from_points(st, n, *args) == INVALID, i
        args[i] = None
        assert lib.dvs_init_from_points(st, n, *args) == INVALID, i
    torch.cuda.synchronize()
