"""dvs_downsample_views (csrc/resample.hip) on the GPU, bit for bit against tests/resolution_ref.py::downsample_np, on the smallest
shapes at which it can go wrong: one block exactly (8x8), even sizes that no factor above 2 divides (70x54: cropped columns and rows),
odd sizes (129x67), more than one workgroup along a row (515x33, 528x16), smaller than a lane's four outputs (7x5), and the two shapes
at which the 16-byte path runs for 8-bit sources (64x24 at every factor; 528x16 at factors 1, 2, 4 and the scalar path at 8) — fp32
sources take it at 8x8, 64x24 and 528x16. Every shape runs with 1, 3 and 16 views, 1 and 3 planes, and both with 16-byte aligned
pointers and with the sources 1 element (1 byte / 4 bytes) and the destinations 4 bytes off a 16-byte boundary, which forces the
scalar path. The bytes around every destination must stay untouched."""
import ctypes as C
import numpy as np
import pytest
from resolution_ref import downsample_np, same_bits
from train_step_ref import pack_unpack_u8

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8), (70, 54), (129, 67), (515, 33), (7, 5), (64, 24), (528, 16)]
INVALID = 1                                                  # DVS_ERR_INVALID
GUARD = 8                                                    # floats kept around every destination


def _sources(seed, V, planes, H, W, u8):
    rng = np.random.default_rng(seed)
    if u8:
        return rng.integers(0, 256, (V, planes, H, W), dtype=np.uint8)
    return (rng.uniform(-1, 2, (V, planes, H, W)) * 10.0 ** rng.integers(-3, 4, (V, planes, H, W))).astype(np.float32)   # rounding depends on the order


def _call(dev, srcs, f, offset):
    """one dvs_downsample_views call on device copies of srcs [V, planes, H, W] -> float32 [V, planes, H // f, W // f]; offset: every
    source starts one element, every destination one float past a 16-byte boundary"""
    import torch
    from divshot_amd._lib import lib, DownsampleView
    V, planes, H, W = srcs.shape
    u8 = srcs.dtype == np.uint8
    n_src, n_dst = planes * H * W, planes * (H // f) * (W // f)
    so, do = (1, GUARD + 1) if offset else (0, GUARD)
    arr = (DownsampleView * V)()
    keep, dsts = [], []
    for v in range(V):
        sb = torch.zeros(n_src + 16, dtype=torch.uint8 if u8 else torch.float32, device=dev)
        db = torch.full((n_dst + 2 * GUARD + 4,), -777.0, dtype=torch.float32, device=dev)
        assert sb.data_ptr() % 16 == 0 and db.data_ptr() % 16 == 0
        sb[so:so + n_src].copy_(torch.from_numpy(srcs[v].reshape(-1)))
        arr[v].src, arr[v].dst = sb.data_ptr() + so * sb.element_size(), db.data_ptr() + do * 4
        assert (arr[v].src % 16 != 0) == offset and (arr[v].dst % 16 != 0) == offset
        keep.append(sb); dsts.append(db)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.dvs_downsample_views(st, arr, V, planes, W, H, f, int(u8)) == 0
    torch.cuda.synchronize()
    out = np.empty((V, planes, H // f, W // f), np.float32)
    for v in range(V):
        h = dsts[v].cpu().numpy()
        assert (h[:do] == -777.0).all() and (h[do + n_dst:] == -777.0).all(), "a write outside the destination"
        out[v] = h[do:do + n_dst].reshape(out[v].shape)
    return out


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("W,H", SHAPES)
def test_bit_exact_against_the_restatement(gpu_device, W, H, u8):
    ran = 0
    for planes in (1, 3):
        srcs = _sources(W * 1000 + H + planes, 16, planes, H, W, u8)
        for f in (1, 2, 4, 8):
            if W // f == 0 or H // f == 0:
                continue
            want = np.stack([downsample_np(s, f) for s in srcs])
            for V in (1, 3, 16):
                for offset in (False, True):
                    got = _call(gpu_device, srcs[:V], f, offset)
                    assert same_bits(got, want[:V]), (W, H, planes, f, V, offset, float(np.abs(got - want[:V]).max()))
                    ran += 1
    assert ran == 2 * 6 * sum(1 for f in (1, 2, 4, 8) if W // f and H // f)


def test_a_view_does_not_depend_on_its_batch_and_calls_repeat(gpu_device):
    for u8 in (True, False):
        srcs = _sources(5, 16, 3, 54, 80, u8)
        full = _call(gpu_device, srcs, 2, False)
        assert full.tobytes() == _call(gpu_device, srcs, 2, False).tobytes()           # two calls: identical bits
        for v in (0, 7, 15):
            alone = _call(gpu_device, srcs[v:v + 1], 2, False)
            assert alone[0].tobytes() == full[v].tobytes(), (u8, v)
        mixed = _call(gpu_device, srcs[[7, 0, 15]], 2, True)                            # other neighbours, the other path
        assert mixed.tobytes() == full[[7, 0, 15]].tobytes()


def test_factor_one_on_bytes_is_the_trainers_expansion(gpu_device):
    rng = np.random.default_rng(2)
    t = rng.uniform(-0.1, 1.1, (1, 3, 21, 35)).astype(np.float32)
    bytes_ = np.rint(np.clip(t * np.float32(255.0), 0, 255)).astype(np.uint8)
    assert len(np.unique(bytes_)) == 256
    for offset in (False, True):
        assert same_bits(_call(gpu_device, bytes_, 1, offset), pack_unpack_u8(t))


def test_python_wrapper(gpu_device):
    import torch
    from divshot_amd.train_ops import downsample_views
    srcs = _sources(9, 2, 3, 33, 47, False)
    outs = downsample_views([torch.tensor(s, device=gpu_device) for s in srcs], 4)
    assert [tuple(o.shape) for o in outs] == [(3, 8, 11)] * 2
    for o, s in zip(outs, srcs):
        assert same_bits(o.cpu().numpy(), downsample_np(s, 4))


def test_argument_checks(gpu_device):
    import torch
    from divshot_amd._lib import lib, DownsampleView
    W, H = 16, 8
    x = torch.zeros((3, H, W), device=gpu_device)
    y = torch.zeros((3, H, W), device=gpu_device)
    arr = (DownsampleView * 17)()
    for a in arr:
        a.src, a.dst = x.data_ptr(), y.data_ptr()
    call = lambda n, planes=3, w=W, h=H, f=2, views=arr: lib.dvs_downsample_views(None, views, n, planes, w, h, f, 0)
    assert call(1) == 0 and call(16) == 0
    assert call(0) == INVALID and call(17) == INVALID and call(-1) == INVALID
    assert call(1, views=None) == INVALID
    assert call(1, planes=0) == INVALID and call(1, planes=-3) == INVALID
    for f in (0, 3, 5, 6, 16, -2):
        assert call(1, f=f) == INVALID, f
    assert call(1, f=8) == 0 and call(1, h=7, f=8) == INVALID and call(1, w=3, f=4) == INVALID        # height / f == 0, width / f == 0
    assert call(1, w=0) == INVALID and call(1, h=-1) == INVALID
    arr[1].src = None
    assert call(2) == INVALID and call(1) == 0                # a NULL src among the views that are used
    arr[1].src, arr[0].dst = x.data_ptr(), None
    assert call(1) == INVALID
    torch.cuda.synchronize()
