"""dvs_png_reconstruct and dvs_mask_combine (csrc/png.hip) on the GPU against tests/png_ref.py, bit for bit. The inputs are RANDOM FILTERED
STREAMS: any bytes with filter bytes in 0..4 are a valid stream, so no encoder is involved and Paeth and Average see arbitrary
neighbours. The shapes are the smallest at which the wavefront can go wrong: 1x1 and 37x29 for every colour type / bit depth pair (the
row filters cycling 0..4 from each of the five starts, so Up, Average and Paeth each land on the first row), the widths that pad a row
to a byte at depths 1, 2, 4, one long chain in each direction at bpp 3, heights that cross the row-band seam by 1 and by band + 1 rows
(the band size is read from the library), the arithmetic corners (a = b = c; 0xFF rows under Average), colour keys that match in the
high byte only, a 3-entry palette under indices up to 255 with a shorter tRNS, alpha = NULL. The filtered buffer, the rgb planes and
the alpha plane sit between guard bytes, and the filtered buffer starts off a 4-byte boundary."""
import ctypes as C
import numpy as np
import pytest
import png_ref as P

pytestmark = pytest.mark.gpu

INVALID = 1
GUARD, FILL = 64, 0xA5


def _frame(width, height, depth, ctype, palette=None, key=None):
    f = P.Frame()
    f.width, f.height, f.depth, f.ctype, f.key = width, height, depth, ctype, key
    if palette is not None:
        f.palette[:] = palette
    return f


def _desc(f):
    from divshot_amd._lib import PngDesc
    d = PngDesc()
    d.width, d.height, d.bit_depth, d.color_type, d.has_key = f.width, f.height, f.depth, f.ctype, 0 if f.key is None else 1
    for k, v in enumerate(f.key or []):
        d.key[k] = v
    for k in range(256):
        for j in range(4):
            d.palette[k][j] = int(f.palette[k, j])
    return d


def _guarded(dev, n, shift=0):
    import torch
    t = torch.full((n + 2 * GUARD + 16,), FILL, dtype=torch.uint8, device=dev)
    return t, t.data_ptr() + GUARD + shift


def _inside(t, n, shift=0):
    h = t.cpu().numpy()
    assert (h[:GUARD + shift] == FILL).all() and (h[GUARD + shift + n:] == FILL).all(), "a write outside the buffer"
    return h[GUARD + shift:GUARD + shift + n].copy()


def _run(dev, f, stream, want_alpha=True, shift=1):
    """-> (unfiltered scanlines [H][rowbytes], rgb [3][H][W], alpha [H][W] or None)"""
    import torch
    from divshot_amd._lib import lib
    desc, p = _desc(f), f.width * f.height
    n = lib.dvs_png_filtered_bytes(C.byref(desc))
    assert n == stream.size == f.height * (1 + P.row_bytes(f.width, f.depth, f.ctype))
    buf, buf_at = _guarded(dev, n, shift)
    buf[GUARD + shift:GUARD + shift + n] = torch.from_numpy(stream).to(dev)
    rgb, rgb_at = _guarded(dev, 3 * p)
    alpha, alpha_at = _guarded(dev, p)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.dvs_png_reconstruct(st, C.byref(desc), buf_at, rgb_at, alpha_at if want_alpha else None) == 0
    torch.cuda.synchronize()
    rows = _inside(buf, n, shift).reshape(f.height, -1)[:, 1:]
    a = _inside(alpha, p)
    if not want_alpha:
        assert (a == FILL).all()
    return rows, _inside(rgb, 3 * p).reshape(3, f.height, f.width), a.reshape(f.height, f.width) if want_alpha else None


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), [int(got[tuple(b)]) for b in bad[:5]], [int(want[tuple(b)]) for b in bad[:5]])


def _check(dev, f, stream, what, want_alpha=True):
    rows = P.unfilter(stream, f.width, f.height, f.depth, f.ctype)
    rgb, alpha = P.expand(rows, f)
    g_rows, g_rgb, g_alpha = _run(dev, f, stream, want_alpha)
    _same(g_rows, rows, what + ": unfiltered scanlines")
    _same(g_rgb, rgb, what + ": rgb")
    if want_alpha:
        _same(g_alpha, alpha, what + ": alpha")
    return g_rgb, g_alpha


def _extras(rng, ctype, depth):
    """a palette with a tRNS for type 3, a key that occurs for types 0 and 2 at small depths"""
    palette = None
    if ctype == 3:
        palette = np.zeros((256, 4), np.uint8)
        palette[:, 3] = 255
        n = min(1 << depth, 200)
        palette[:n, :3] = rng.integers(0, 256, (n, 3))
        palette[:n // 2, 3] = rng.integers(0, 256, n // 2)
    key = {0: [1], 2: [1, 2, 3]}.get(ctype)
    return palette, key


@pytest.mark.parametrize("ctype,depth", P.PAIRS)
def test_1x1_every_pair(gpu_device, ctype, depth):
    rng = np.random.default_rng(7 + 100 * ctype + depth)
    palette, key = _extras(rng, ctype, depth)
    for ft in range(5):
        f = _frame(1, 1, depth, ctype, palette, key)
        _check(gpu_device, f, P.random_stream(rng, 1, 1, depth, ctype, filters=[ft]), f"1x1 type {ctype} depth {depth} filter {ft}")


@pytest.mark.parametrize("ctype,depth", P.PAIRS)
def test_37x29_every_pair_every_filter_on_the_first_row(gpu_device, ctype, depth):
    rng = np.random.default_rng(11 + 100 * ctype + depth)
    palette, key = _extras(rng, ctype, depth)
    for start in range(5):
        f = _frame(37, 29, depth, ctype, palette, key)
        stream = P.random_stream(rng, 37, 29, depth, ctype, filters=[(y + start) % 5 for y in range(29)])
        _, alpha = _check(gpu_device, f, stream, f"37x29 type {ctype} depth {depth} start {start}")
        if ctype in (3, 4, 6) or (ctype == 0 and depth <= 4):
            assert alpha.min() < 255                                         # the alpha rule was exercised, not only its default


@pytest.mark.parametrize("depth", [1, 2, 4])
@pytest.mark.parametrize("width", [1, 7, 8, 9, 13])
def test_row_padding_bits(gpu_device, width, depth):
    rng = np.random.default_rng(1000 + 16 * width + depth)
    for ctype in (0, 3):
        palette, key = _extras(rng, ctype, depth)
        f = _frame(width, 6, depth, ctype, palette, key)
        _check(gpu_device, f, P.random_stream(rng, width, 6, depth, ctype), f"{width}x6 type {ctype} depth {depth}")


@pytest.mark.parametrize("width,height", [(3000, 2), (2, 3000)])
def test_a_long_chain_in_each_direction_at_bpp_3(gpu_device, width, height):
    rng = np.random.default_rng(width)
    f = _frame(width, height, 8, 2)
    _check(gpu_device, f, P.random_stream(rng, width, height, 8, 2, filters=[(3, 4, 1, 2)[y % 4] for y in range(height)]), f"{width}x{height}")


def test_heights_across_the_band_seam_all_paeth(gpu_device):
    from divshot_amd._lib import lib
    band = lib.dvs_png_band_rows()
    assert 1 <= band <= 4096
    rng = np.random.default_rng(5)
    for height in (band + 1, 2 * band + 1):
        f = _frame(5, height, 8, 2)
        _check(gpu_device, f, P.random_stream(rng, 5, height, 8, 2, filters=[4] * height), f"5x{height} Paeth")


def test_constant_rows_and_ff_rows_under_average(gpu_device):
    w, h = 21, 8
    for ctype, depth in ((2, 8), (0, 8), (6, 16)):
        rb = P.row_bytes(w, depth, ctype)
        unf = np.full((h, rb), 0x5C, np.uint8)                               # a = b = c everywhere past the first row and column
        f = _frame(w, h, depth, ctype)
        for ft in range(5):
            rows, _, _ = _run(gpu_device, f, P.filter_rows(unf, w, h, depth, ctype, [ft]))
            _same(rows, unf, f"constant rows, filter {ft}")
        stream = np.full((h, rb + 1), 0xFF, np.uint8)                        # 0xFF under Average: a + b reaches 510, the 9-bit sum
        stream[:, 0] = 3
        _check(gpu_device, f, stream.reshape(-1), f"0xFF rows under Average, type {ctype}")
        unf = np.full((h, rb), 0xFF, np.uint8)
        rows, _, _ = _run(gpu_device, f, P.filter_rows(unf, w, h, depth, ctype, [3]))
        _same(rows, unf, "rows that unfilter to 0xFF under Average")


def test_16_bit_keys_that_match_in_the_high_byte_only(gpu_device):
    rng = np.random.default_rng(9)
    w, h = 37, 5
    for ctype, key in ((0, [0x1234]), (2, [0x1234, 0xABCD, 0x00FF])):
        ch = P.CHANNELS[ctype]
        s = rng.integers(0, 65536, (h, w, ch))
        s[0, :, :] = key                                                     # the key itself: transparent
        s[1, :, :] = [(k & 0xFF00) | ((k + 1) & 0xFF) for k in key]          # the high bytes only: opaque
        s[2, :, :] = key
        s[2, :, ch - 1] ^= 0x0100                                            # the last channel differs in its high byte only: opaque
        f = _frame(w, h, 16, ctype, key=key)
        stream = P.filter_rows(P.pack_samples(s.reshape(h, w * ch), 16), w, h, 16, ctype, [0, 4, 3, 1, 2])
        _, alpha = _check(gpu_device, f, stream, f"16-bit key, type {ctype}")
        assert (alpha[0] == 0).all() and (alpha[1] == 255).all() and (alpha[2] == 255).all()


def test_a_3_entry_palette_under_indices_up_to_255(gpu_device):
    rng = np.random.default_rng(13)
    palette = np.zeros((256, 4), np.uint8)
    palette[:, 3] = 255                                                      # the padding: opaque black
    palette[:3, :3] = [[10, 20, 30], [40, 50, 60], [70, 80, 90]]
    palette[:2, 3] = [0, 128]                                                # a tRNS shorter than the palette
    f = _frame(37, 29, 8, 3, palette)
    stream = P.random_stream(rng, 37, 29, 8, 3)
    rgb, alpha = _check(gpu_device, f, stream, "3-entry palette")
    idx = P.unfilter(stream, 37, 29, 8, 3)
    assert idx.max() > 200 and (rgb[:, idx > 2] == 0).all() and (alpha[idx > 2] == 255).all() and (alpha[idx == 1] == 128).all()


def test_alpha_null_gives_the_same_rgb(gpu_device):
    rng = np.random.default_rng(17)
    for ctype, depth in ((6, 8), (4, 16), (2, 8)):
        f = _frame(37, 29, depth, ctype)
        stream = P.random_stream(rng, 37, 29, depth, ctype)
        with_alpha, _ = _check(gpu_device, f, stream, "with alpha")
        without, none = _check(gpu_device, f, stream, "alpha = NULL", want_alpha=False)
        assert none is None
        _same(without, with_alpha, "rgb with and without alpha")


def test_invalid_arguments(gpu_device):
    import torch
    from divshot_amd._lib import lib
    f = _frame(8, 8, 8, 2)
    buf = torch.zeros(4096, dtype=torch.uint8, device=gpu_device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = buf.data_ptr()
    good = _desc(f)
    assert lib.dvs_png_filtered_bytes(C.byref(good)) == 8 * 25
    assert lib.dvs_png_reconstruct(st, None, p, p + 1024, None) == INVALID
    assert lib.dvs_png_reconstruct(st, C.byref(good), None, p + 1024, None) == INVALID
    assert lib.dvs_png_reconstruct(st, C.byref(good), p, None, None) == INVALID
    assert lib.dvs_png_filtered_bytes(None) == 0
    for field, value in (("width", 0), ("height", 0), ("width", 65501), ("height", -1), ("bit_depth", 4), ("bit_depth", 3), ("color_type", 5),
                         ("color_type", 1), ("has_key", 2)):
        d = _desc(f)
        setattr(d, field, value)
        assert lib.dvs_png_filtered_bytes(C.byref(d)) == 0, (field, value)
        assert lib.dvs_png_reconstruct(st, C.byref(d), p, p + 1024, None) == INVALID, (field, value)
    for ctype, depth in ((3, 16), (4, 4), (6, 2), (2, 1)):
        d = _desc(_frame(8, 8, 8, 2))
        d.color_type, d.bit_depth = ctype, depth
        assert lib.dvs_png_reconstruct(st, C.byref(d), p, p + 1024, None) == INVALID, (ctype, depth)
    for ctype in (3, 4, 6):                                                  # a key beside a palette or an alpha channel contradicts itself
        d = _desc(_frame(8, 8, 8, ctype))
        d.has_key = 1
        assert lib.dvs_png_reconstruct(st, C.byref(d), p, p + 1024, None) == INVALID, ctype
    assert lib.dvs_mask_combine(st, 64, None, None, None, p, None) == INVALID
    assert lib.dvs_mask_combine(st, 64, p, None, None, None, None) == INVALID
    assert lib.dvs_mask_combine(st, 0, p, None, None, p + 1024, None) == INVALID
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0).all()                                    # nothing was launched


@pytest.mark.parametrize("use_alpha", [False, True])
@pytest.mark.parametrize("use_other", [False, True])
@pytest.mark.parametrize("outputs", ["u8", "f32", "both"])
def test_mask_combine(gpu_device, use_alpha, use_other, outputs):
    import torch
    from divshot_amd._lib import lib
    w, h = 37, 29
    n = w * h
    rng = np.random.default_rng(21)
    values = np.array([0, 127, 128, 255], np.uint8)
    gray, alpha, other = values[rng.integers(0, 4, n)], values[rng.integers(0, 4, n)], rng.integers(0, 2, n).astype(np.uint8)
    want = gray > 127
    if use_alpha:
        want = want & (alpha > 127)
    if use_other:
        want = want & (other != 0)
    assert 0 < want.sum() < n
    d = [torch.from_numpy(a).to(gpu_device) for a in (gray, alpha, other)]
    out8, out8_at = _guarded(gpu_device, n)
    out32 = torch.full((n + 32,), -1.0, dtype=torch.float32, device=gpu_device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.dvs_mask_combine(st, n, d[0].data_ptr(), d[1].data_ptr() if use_alpha else None, d[2].data_ptr() if use_other else None,
                                out8_at if outputs != "f32" else None, out32.data_ptr() + 64 if outputs != "u8" else None) == 0
    torch.cuda.synchronize()
    got8, got32 = _inside(out8, n), out32.cpu().numpy()
    assert np.array_equal(got8, want.astype(np.uint8) if outputs != "f32" else np.full(n, FILL, np.uint8))
    assert (got32[:16] == -1).all() and (got32[16 + n:] == -1).all()
    assert np.array_equal(got32[16:16 + n], want.astype(np.float32) if outputs != "u8" else np.full(n, -1, np.float32))
    if outputs == "both" and use_other:                                      # the converter form: no gray plane, a {0, 1} plane in
        assert lib.dvs_mask_combine(st, n, None, None, d[2].data_ptr(), None, out32.data_ptr() + 64) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out32.cpu().numpy()[16:16 + n], other.astype(np.float32))
