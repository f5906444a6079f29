"""PNG restated in numpy and the standard library's zlib (no PIL): a writer that builds every case the tests need without committing
binaries, and the reference decoder that divshot_amd/gstrain/png_io.cpp (chunk parsing, inflate: `decode_filtered`) and
dvs_png_reconstruct (the five filters, sample expansion: `unfilter`, `expand`) are held against bit for bit. include/dvs_image.h states
the rules; this file follows them one for one."""
import struct
import zlib
import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
PAIRS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def row_bytes(width, depth, ctype):
    return (width * CHANNELS[ctype] * depth + 7) // 8


def bpp_of(depth, ctype):
    return max(1, CHANNELS[ctype] * depth // 8)


def chunk(ctype, body=b"", crc=None):
    """one chunk; `crc` overrides the computed CRC-32"""
    body = bytes(body)
    c = zlib.crc32(ctype + body) & 0xFFFFFFFF if crc is None else crc
    return struct.pack(">I", len(body)) + ctype + body + struct.pack(">I", c)


def ihdr(width, height, depth, ctype, compression=0, filter_method=0, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, ctype, compression, filter_method, interlace))


def split_idat(z, split):
    """the IDAT chunks of the zlib stream `z`: split = None for one chunk, an int for pieces of that many bytes, a list for cut points"""
    if split is None:
        return chunk(b"IDAT", z)
    cuts = list(range(split, len(z), split)) if isinstance(split, int) else list(split)
    parts, at = [], 0
    for c in cuts + [len(z)]:
        parts.append(z[at:c])
        at = c
    return b"".join(chunk(b"IDAT", p) for p in parts)


def random_stream(rng, width, height, depth, ctype, filters=None):
    """a valid filtered stream: any bytes with filter bytes in 0..4 (filters: one per row, default random)"""
    rb = row_bytes(width, depth, ctype)
    s = rng.integers(0, 256, (height, rb + 1), dtype=np.uint8)
    s[:, 0] = rng.integers(0, 5, height) if filters is None else np.asarray(filters, np.uint8)
    return s.reshape(-1)


def filter_rows(raw, width, height, depth, ctype, filters):
    """the encoder's direction: unfiltered scanlines [H][rowbytes] -> the filtered stream, with the given per-row filter choice"""
    rb, bpp = row_bytes(width, depth, ctype), bpp_of(depth, ctype)
    raw = np.asarray(raw, np.uint8).reshape(height, rb).astype(np.int32)
    out = np.zeros((height, rb + 1), np.uint8)
    zero = np.zeros(rb, np.int32)
    left = lambda row: np.concatenate([np.zeros(bpp, np.int32), row])[:rb]      # the row moved bpp bytes to the right
    for y in range(height):
        ft = int(filters[y % len(filters)])
        a, b, c = left(raw[y]), (raw[y - 1] if y else zero), (left(raw[y - 1]) if y else zero)
        pred = [zero, a, b, (a + b) >> 1, _paeth(a, b, c)][ft]
        out[y, 0] = ft
        out[y, 1:] = (raw[y] - pred) & 255
    return out.reshape(-1)


def write_png(width, height, depth, ctype, stream, palette=None, trns=None, split=None, extra_before_idat=b"", level=6,
              interlace=0, compression=0, filter_method=0):
    """a PNG file as bytes. stream: the filtered stream (a raw override: whatever bytes are given are deflated as they are);
    palette: [n][3] uint8 (PLTE); trns: bytes of the tRNS chunk; split: see split_idat; extra_before_idat: chunks put after PLTE / tRNS"""
    out = SIG + ihdr(width, height, depth, ctype, compression, filter_method, interlace)
    if palette is not None:
        out += chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    out += extra_before_idat
    out += split_idat(zlib.compress(np.asarray(stream, np.uint8).tobytes(), level), split)
    return out + chunk(b"IEND")


def pack_samples(samples, depth):
    """[H][W*channels] integer samples at `depth` bits -> unfiltered scanlines [H][rowbytes] (MSB first, rows padded to a byte, 16 bits
    big-endian)"""
    s = np.asarray(samples)
    h, n = s.shape
    if depth == 8:
        return s.astype(np.uint8)
    if depth == 16:
        return np.stack([s >> 8, s & 255], -1).astype(np.uint8).reshape(h, 2 * n)
    bits = ((s[..., None] >> np.arange(depth - 1, -1, -1)) & 1).astype(np.uint8).reshape(h, n * depth)
    return np.packbits(bits, axis=1)


def write_image(width, height, depth, ctype, samples, filters=(0, 1, 2, 3, 4), **kw):
    """a PNG file of the given samples ([H][W*channels] at `depth` bits), rows filtered with `filters` in turn"""
    raw = pack_samples(samples, depth)
    return write_png(width, height, depth, ctype, filter_rows(raw, width, height, depth, ctype, filters), **kw)


# ---- the reference decoder ----
class Frame:
    """what gspng::decode_filtered returns: the descriptor and the filtered stream"""
    def __init__(self):
        self.width = self.height = self.depth = self.ctype = 0
        self.palette = np.zeros((256, 4), np.uint8)
        self.palette[:, 3] = 255
        self.key = None
        self.filtered = None


def decode_filtered(data):
    """chunk parse and inflate of a VALID file (the refusals are png_io.cpp's to make; here they are plain assertions)"""
    assert data[:8] == SIG
    f, at, idat, n_plte = Frame(), 8, b"", 0
    while True:
        n, ctype = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert zlib.crc32(ctype + body) & 0xFFFFFFFF == struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0]
        at += 12 + n
        if ctype == b"IHDR":
            f.width, f.height, f.depth, f.ctype, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            assert (f.ctype, f.depth) in PAIRS and comp == 0 and filt == 0 and lace == 0
        elif ctype == b"PLTE":
            n_plte = n // 3
            if f.ctype == 3:
                f.palette[:n_plte, :3] = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif ctype == b"tRNS":
            if f.ctype == 3:
                assert n <= n_plte
                f.palette[:n, 3] = np.frombuffer(body, np.uint8)
            else:
                f.key = list(struct.unpack(">%dH" % (n // 2), body))
        elif ctype == b"IDAT":
            idat += body
        elif ctype == b"IEND":
            break
    f.filtered = np.frombuffer(zlib.decompress(idat), np.uint8).copy()
    assert f.filtered.size == f.height * (1 + row_bytes(f.width, f.depth, f.ctype))
    return f


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def unfilter(filtered, width, height, depth, ctype):
    """the five filters undone: filtered stream -> scanlines [H][rowbytes]. The byte lanes of a pixel are independent, so a row is walked
    pixel by pixel with the bpp lanes as a vector; a filter byte above 4 counts as None"""
    rb, bpp = row_bytes(width, depth, ctype), bpp_of(depth, ctype)
    s = np.asarray(filtered, np.uint8).reshape(height, rb + 1)
    npx = -(-rb // bpp)
    out = np.zeros((height + 1, (npx + 1) * bpp), np.int32)             # a zero row above and a zero pixel to the left
    for y in range(height):
        ft = int(s[y, 0])
        x = np.zeros(npx * bpp, np.int32)
        x[:rb] = s[y, 1:]
        x = x.reshape(npx, bpp)
        cur, up = out[y + 1].reshape(npx + 1, bpp), out[y].reshape(npx + 1, bpp)
        if ft == 2:
            cur[1:] = (x + up[1:]) & 255
        elif ft in (1, 3, 4):
            for i in range(npx):
                a, b, c = cur[i], up[i + 1], up[i]
                pred = a if ft == 1 else (a + b) >> 1 if ft == 3 else _paeth(a, b, c)
                cur[i + 1] = (x[i] + pred) & 255
        else:
            cur[1:] = x
        out[y + 1, bpp + rb:] = 0                                        # the lanes past the row's end are not part of it
    return out[1:, bpp:bpp + rb].astype(np.uint8)


def samples_of(rows, width, depth, ctype):
    """scanlines [H][rowbytes] -> integer samples [H][W][channels] at the file's depth"""
    ch, h = CHANNELS[ctype], rows.shape[0]
    if depth == 8:
        return rows[:, :width * ch].astype(np.int64).reshape(h, width, ch)
    if depth == 16:
        r = rows.astype(np.int64).reshape(h, width * ch, 2)
        return (r[..., 0] << 8 | r[..., 1]).reshape(h, width, ch)
    bits = np.unpackbits(rows, axis=1)[:, :width * depth].reshape(h, width, depth).astype(np.int64)
    return (bits << np.arange(depth - 1, -1, -1)).sum(-1)[..., None]


def expand(rows, frame):
    """-> (rgb uint8 [3][H][W], alpha uint8 [H][W]) by the rules of include/dvs_image.h"""
    w, depth, ctype = frame.width, frame.depth, frame.ctype
    s = samples_of(rows, w, depth, ctype)
    v = (s * 255 + 32895) >> 16 if depth == 16 else s * {1: 255, 2: 85, 4: 17, 8: 1}[depth]
    alpha = np.full(s.shape[:2], 255, np.int64)
    if ctype == 3:
        e = frame.palette[s[..., 0]].astype(np.int64)
        rgb, alpha = e[..., :3], e[..., 3]
    elif ctype in (0, 4):
        rgb = np.repeat(v[..., :1], 3, -1)
        if ctype == 4:
            alpha = v[..., 1]
    else:
        rgb = v[..., :3]
        if ctype == 6:
            alpha = v[..., 3]
    if frame.key is not None and ctype in (0, 2):
        mask = 0xFFFF if depth == 16 else (1 << depth) - 1
        key = np.array([k & mask for k in frame.key[:CHANNELS[ctype]]], np.int64)
        alpha = np.where((s[..., :len(key)] == key).all(-1), 0, 255)
    return np.ascontiguousarray(rgb.transpose(2, 0, 1)).astype(np.uint8), alpha.astype(np.uint8)


def decode(data):
    """a file -> (rgb [3][H][W], alpha [H][W])"""
    f = decode_filtered(data)
    return expand(unfilter(f.filtered, f.width, f.height, f.depth, f.ctype), f)
