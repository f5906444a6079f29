"""Writes tests/golden/jpeg/*.jpg and tests/golden/jpeg_expected.npz. Run once, by hand, where PIL is installed; no test imports PIL.
Per fixture the npz holds the PIL-decoded pixels (`<name>/pil`, uint8 [3][H][W]), the pixels of tests/jpeg_ref.py's integer pipeline
(`<name>/int`) and of its fp64-IDCT variant (`<name>/fp64`), and the measured max abs difference of each to PIL (`<name>/d_int`,
`<name>/d_fp64`). Files that must be rejected (progressive, adobe_rgb) have no entry."""
import io
import os
import struct
import sys
import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_ref as J  # noqa: E402

OUT = os.path.join(HERE, "jpeg")


def picture(w, h, seed):
    """smooth colour ramps, one hard edge and a little noise: every frequency band gets something"""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 100 * np.sin(x / (3.0 + seed) + y / 7.0), 128 + 90 * np.cos(y / (2.5 + seed) - x / 9.0), 255.0 * ((x + 2 * y) % 23 < 11)], axis=2)
    img += r.normal(0, 6, img.shape)
    img[h // 3:, w // 2:] = img[h // 3:, w // 2:][::-1, ::-1] * 0.6 + 40
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def encode(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def segments(data):
    """-> [(marker, start, end)] of the segments before the scan"""
    out, pos = [], 2
    while data[pos + 1] != 0xDA:
        L = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        out.append((data[pos + 1], pos, pos + 2 + L))
        pos += 2 + L
    return out


def with_16bit_dqt(data):
    """every DQT table rewritten with 16-bit entries (Pq = 1), the values unchanged"""
    out, last = bytearray(), 0
    for m, a, b in segments(data):
        if m != 0xDB:
            continue
        body, new, at = data[a + 4:b], bytearray(), 0
        while at < len(body):
            assert body[at] >> 4 == 0
            new += bytes([0x10 | body[at]]) + b"".join(struct.pack(">H", v) for v in body[at + 1:at + 65])
            at += 65
        out += data[last:a] + b"\xff\xdb" + struct.pack(">H", len(new) + 2) + new
        last = b
    return bytes(out + data[last:])


def with_adobe_rgb(data):
    """an APP14 "Adobe" segment with transform byte 0 right after SOI: the three components are then R, G, B"""
    return data[:2] + b"\xff\xee" + struct.pack(">H", 14) + b"Adobe" + struct.pack(">HHHB", 100, 0, 0, 0) + data[2:]


def main():
    os.makedirs(OUT, exist_ok=True)
    files = {}
    for (w, h) in ((37, 29), (40, 24)):
        for sub, name in ((0, "444"), (1, "422"), (2, "420")):
            files[f"c{name}_{w}x{h}"] = encode(picture(w, h, 1 + sub), quality=90, subsampling=sub)
    files["c420_40x24_opt"] = encode(picture(40, 24, 5), quality=85, subsampling=2, optimize=True)
    files["c420_40x24_rst3"] = encode(picture(40, 24, 6), quality=85, subsampling=2, restart_marker_blocks=3)
    files["gray_37x29"] = encode(picture(37, 29, 7)[:, :, 0], quality=90)
    files["q100_37x29"] = encode(picture(37, 29, 8), quality=100, subsampling=2)
    files["q5_37x29"] = encode(picture(37, 29, 9), quality=5, subsampling=2)
    files["s_8x8"] = encode(picture(8, 8, 10), quality=90, subsampling=2)
    files["s_1x1"] = encode(picture(1, 1, 11), quality=90, subsampling=2)
    files["s_17x1"] = encode(picture(17, 1, 12), quality=90, subsampling=2)
    files["dqt16_40x24"] = with_16bit_dqt(files["c420_40x24"])
    rejected = {"progressive": encode(picture(37, 29, 13), quality=90, subsampling=2, progressive=True),
                "adobe_rgb": with_adobe_rgb(files["c444_37x29"])}
    expected = {}
    for name, data in files.items():
        assert len(data) < 8192, (name, len(data))
        pil = np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).transpose(2, 0, 1).copy()
        frame = J.decode_coefficients(data)
        assert J.clamped_count(frame) == 0, name
        a, b = J.reconstruct(frame), J.reconstruct(frame, "fp64")
        assert a.shape == pil.shape, (name, a.shape, pil.shape)
        d_int = int(np.abs(a.astype(int) - pil.astype(int)).max())
        d_fp = int(np.abs(b.astype(int) - pil.astype(int)).max())
        print(f"{name}: {len(data)} bytes, {frame.width}x{frame.height}, luma {frame.hs[0]}x{frame.vs[0]}, |int - PIL| <= {d_int}, |fp64 - PIL| <= {d_fp}")
        expected.update({f"{name}/pil": pil, f"{name}/int": a, f"{name}/fp64": b, f"{name}/d_int": np.int64(d_int), f"{name}/d_fp64": np.int64(d_fp)})
    for name, data in list(files.items()) + list(rejected.items()):
        open(os.path.join(OUT, name + ".jpg"), "wb").write(data)
    for name, data in rejected.items():
        try:
            J.decode_coefficients(data)
        except ValueError as e:
            print(f"{name}: rejected: {e}")
        else:
            raise AssertionError(name + " was accepted")
    assert files["dqt16_40x24"] != files["c420_40x24"] and np.array_equal(expected["dqt16_40x24/int"], expected["c420_40x24/int"])
    np.savez_compressed(os.path.join(HERE, "jpeg_expected.npz"), **expected)


if __name__ == "__main__":
    main()
