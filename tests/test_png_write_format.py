"""gspng::write_png (divshot_amd/gstrain/png_io.cpp) through libgsplyio.so, on the CPU: the file's chunk order, lengths and CRCs; the
IDAT bodies concatenated and inflated by Python's zlib are the stream; a stream above 1 MiB at level 0 splits into several IDAT chunks
of at most 1 MiB; the tEXt chunks are there; png_ref.decode and the project's own decoder (gstrain_png_open_memory) both give the stream
and the samples back; PIL, where it is installed, opens the three kinds with equal pixels; every refusal is a message and no output."""
import struct
import zlib
import numpy as np
import pytest
import png_enc_ref as PE
import png_ref

MAX_IDAT = 1 << 20


def lib():
    from divshot_amd import _lib
    return _lib


def chunks(data):
    """-> [(type, body)] of a file whose signature and every CRC hold"""
    assert data[:8] == png_ref.SIG
    out, at = [], 8
    while at < len(data):
        n, ctype = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert len(body) == n and zlib.crc32(ctype + body) & 0xFFFFFFFF == struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0], ctype
        out.append((ctype, body))
        at += 12 + n
    assert at == len(data)
    return out


def stream_of(W, H, kind, scale=255.0, seed=1):
    img = PE.image(W, H, seed)
    return PE.encode(PE.plane_of(img, kind), scale, kind)[0], PE.raw_rows(PE.plane_of(img, kind), scale, kind)[0]


@pytest.mark.parametrize("kind", PE.KINDS, ids=["rgb8", "gray8", "gray16"])
@pytest.mark.parametrize("shape", [(1, 1), (17, 5), (64, 48), (257, 9)], ids=lambda s: "%dx%d" % s)
def test_chunks_crcs_idat_and_both_decoders(shape, kind):
    W, H = shape
    ctype, depth = PE.PNG_TYPE[kind]
    stream, raw = stream_of(W, H, kind, 1000.0 if kind == PE.GRAY16 else 255.0)
    for level, text in ((6, [("depth_scale", "1000"), ("Comment", "caf\xe9")]), (0, None), (9, None)):
        data = lib().png_write(W, H, depth, ctype, stream, level=level, text=text)
        ch = chunks(data)
        names = [c for c, _ in ch]
        n_text = len(text or [])
        assert names[0] == b"IHDR" and names[1:1 + n_text] == [b"tEXt"] * n_text and names[-1] == b"IEND" and ch[-1][1] == b""
        assert set(names[1 + n_text:-1]) == {b"IDAT"} and all(0 < len(b) <= MAX_IDAT for c, b in ch if c == b"IDAT")
        assert ch[0][1] == struct.pack(">IIBBBBB", W, H, depth, ctype, 0, 0, 0)
        if text:
            assert [b for c, b in ch if c == b"tEXt"] == [b"depth_scale\x001000", b"Comment\x00caf\xe9"]
        assert zlib.decompress(b"".join(b for c, b in ch if c == b"IDAT")) == stream.tobytes()
        # the restated decoder
        f = png_ref.decode_filtered(data)
        assert (f.width, f.height, f.depth, f.ctype) == (W, H, depth, ctype) and np.array_equal(f.filtered, stream)
        rows = png_ref.unfilter(f.filtered, W, H, depth, ctype)
        assert np.array_equal(rows, raw)
        rgb, alpha = png_ref.decode(data)
        assert rgb.shape == (3, H, W) and (alpha == 255).all()
        # the project's own decoder
        desc, filtered = lib().png_decode_filtered(data)
        assert (desc.width, desc.height, desc.bit_depth, desc.color_type, desc.has_key) == (W, H, depth, ctype, 0)
        assert np.array_equal(filtered, stream)
        samples = png_ref.samples_of(rows, W, depth, ctype)
        want = PE.quantise(PE.plane_of(PE.image(W, H, 1), kind), 1000.0 if kind == PE.GRAY16 else 255.0, kind)[0]
        assert np.array_equal(samples, want.transpose(1, 2, 0) if kind == PE.RGB8 else want[..., None])


def test_a_stream_above_one_mebibyte_at_level_0_splits_into_several_idat_chunks():
    W, H = 700, 520
    stream = png_ref.random_stream(np.random.default_rng(5), W, H, 8, 2)
    assert stream.size > MAX_IDAT
    data = lib().png_write(W, H, 8, 2, stream, level=0)
    idat = [b for c, b in chunks(data) if c == b"IDAT"]
    assert len(idat) >= 2 and all(len(b) <= MAX_IDAT for b in idat) and len(idat[0]) == MAX_IDAT
    assert zlib.decompress(b"".join(idat)) == stream.tobytes()
    assert np.array_equal(lib().png_decode_filtered(data)[1], stream)
    small = lib().png_write(W, H, 8, 2, np.zeros_like(stream), level=6)
    assert len(small) < 4096 and len([1 for c, _ in chunks(small) if c == b"IDAT"]) == 1


def test_pil_opens_the_three_kinds_with_equal_pixels(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    W, H = 37, 11
    for kind, mode in ((PE.RGB8, "RGB"), (PE.GRAY8, "L"), (PE.GRAY16, "I;16")):
        ctype, depth = PE.PNG_TYPE[kind]
        scale = 65535.0 if kind == PE.GRAY16 else 255.0
        img = PE.plane_of(PE.image(W, H, 4), kind)
        path = str(tmp_path / f"k{kind}.png")
        open(path, "wb").write(lib().png_write(W, H, depth, ctype, PE.encode(img, scale, kind)[0], text=[("depth_scale", "65535")]))
        with Image.open(path) as im:
            im.load()
            assert im.size == (W, H) and im.mode in (mode, "I;16B", "I"), im.mode
            got = np.asarray(im).astype(np.int64)
            assert im.info.get("depth_scale") == "65535"
        want = PE.quantise(img, scale, kind)[0]
        assert np.array_equal(got, want.transpose(1, 2, 0) if kind == PE.RGB8 else want)


def test_every_refusal_is_a_message_and_no_output():
    import ctypes as C
    L = lib()
    h = L.host_lib()
    W, H = 5, 4
    stream = png_ref.random_stream(np.random.default_rng(2), W, H, 8, 2)

    def call(ints, data, size, keys=(), texts=(), null_stream=False, null_size=False):
        out, n_out, err = np.full(4096, 0xAB, np.uint8), C.c_uint64(77), C.create_string_buffer(512)
        k = (C.c_char_p * max(1, len(keys)))(*keys)
        t = (C.c_char_p * max(1, len(texts)))(*texts)
        rc = h.gstrain_png_write((C.c_int32 * 5)(*ints), None if null_stream else data.ctypes.data, size, k, t, len(keys), out.ctypes.data, out.size,
                                 None if null_size else C.byref(n_out), err, 512)
        return rc, n_out.value, err.value.decode("latin-1"), out

    rc, n, msg, out = call((W, H, 8, 2, 6), stream, stream.size)
    assert rc == 0 and n > 0 and msg == "" and bytes(out[:8]) == png_ref.SIG
    bad5 = stream.copy()
    bad5[2 * (1 + 3 * W)] = 5
    cases = [("NULL stream", dict(ints=(W, H, 8, 2, 6), data=stream, size=stream.size, null_stream=True), "NULL"),
             ("type 2 at depth 4", dict(ints=(W, H, 4, 2, 6), data=stream, size=stream.size), "pair"),
             ("type 5", dict(ints=(W, H, 8, 5, 6), data=stream, size=stream.size), "pair"),
             ("depth 16 stream length", dict(ints=(W, H, 16, 2, 6), data=stream, size=stream.size), "bytes"),
             ("width 0", dict(ints=(0, H, 8, 2, 6), data=stream, size=stream.size), "size"),
             ("height 65501", dict(ints=(W, 65501, 8, 2, 6), data=stream, size=stream.size), "size"),
             ("a byte short", dict(ints=(W, H, 8, 2, 6), data=stream, size=stream.size - 1), "bytes"),
             ("a row short", dict(ints=(W, H + 1, 8, 2, 6), data=stream, size=stream.size), "bytes"),
             ("filter byte 5", dict(ints=(W, H, 8, 2, 6), data=bad5, size=bad5.size), "filter type 5"),
             ("level -1", dict(ints=(W, H, 8, 2, -1), data=stream, size=stream.size), "level"),
             ("level 10", dict(ints=(W, H, 8, 2, 10), data=stream, size=stream.size), "level"),
             ("empty keyword", dict(ints=(W, H, 8, 2, 6), data=stream, size=stream.size, keys=[b""], texts=[b"v"]), "keyword"),
             ("80-byte keyword", dict(ints=(W, H, 8, 2, 6), data=stream, size=stream.size, keys=[b"k" * 80], texts=[b"v"]), "keyword"),
             ("control character", dict(ints=(W, H, 8, 2, 6), data=stream, size=stream.size, keys=[b"a\tb"], texts=[b"v"]), "keyword"),
             ("0xA0", dict(ints=(W, H, 8, 2, 6), data=stream, size=stream.size, keys=[b"\xa0"], texts=[b"v"]), "keyword"),
             ("leading space", dict(ints=(W, H, 8, 2, 6), data=stream, size=stream.size, keys=[b" a"], texts=[b"v"]), "keyword")]
    for what, kw, word in cases:
        rc, n, msg, out = call(**kw)
        assert rc != 0 and n == 0 and word in msg and (out == 0xAB).all(), (what, rc, n, msg)
    assert call((W, H, 8, 2, 6), stream, stream.size, null_size=True)[0] != 0
    # the longest legal keyword passes, and the helper raises what the writer says
    assert chunks(L.png_write(W, H, 8, 2, stream, text=[("k" * 79, "")]))[1] == (b"tEXt", b"k" * 79 + b"\x00")
    with pytest.raises(L.DvsError, match="level"):
        L.png_write(W, H, 8, 2, stream, level=11)
