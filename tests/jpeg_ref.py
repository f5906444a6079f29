"""Baseline JPEG, restated from the format's definition (ITU-T T.81) in numpy: the yardstick of divshot_amd/gstrain/jpeg_io.cpp (markers,
Huffman entropy decoding -> coefficients) and of divshot_amd/csrc/jpeg.hip (coefficients -> pixels). Imports numpy and the standard
library only.

decode_coefficients(bytes) -> Frame: what gsjpeg::decode_coefficients returns, field for field. Accepted: SOF0 / SOF1 at 8 bits, 8- or
16-bit DQT, DRI + RST0-7, any Huffman tables, ONE interleaved scan, grayscale or YCbCr with luma 1x1 / 2x1 / 2x2 and chroma 1x1.
Everything else raises ValueError with a message that names the kind.

reconstruct(frame) -> uint8 [3][H][W], defined bit for bit in integer arithmetic (every intermediate fits int32; computed here in
int64 with the int32 range asserted at each step):
  dequantise   F = clamp(coef * q, -2048, 2047)                 (|coef * q| <= 32768 * 65535 < 2^31; an 8-bit image's DCT coefficients
                                                                 lie in [-1024, 1016] and a quantised one comes back within q / 2 of
                                                                 its value, zero once q > 2048: a real encoder's stream never clamps)
  inverse DCT  T[u][x] = round(2^13 * C(u) / 2 * cos((2x + 1) u pi / 16)),  C(0) = 1 / sqrt(2), C(u > 0) = 1      (ONE table, IDCT_T)
               col[y][u] = (sum_v T[v][y] * F[v][u] + 2^8) >> 9           (columns first; 4 fractional bits kept; |col| < 2^17)
               s[y][x]   = (sum_u col[y][u] * T[u][x] + 2^16) >> 17       (then rows; >> is the arithmetic shift)
               sample    = clamp(s + 128, 0, 255)
  upsampling   the triangle filter of the common decoders, over the chroma plane cropped to cw = ceil(W / 2) columns (and, 2x2,
               ch = ceil(H / 2) rows); an index outside [0, cw - 1] or [0, ch - 1] is clamped into it (edge replication):
               2x1: out[2i] = (3 s[i] + s[i-1] + 1) >> 2, out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2
               2x2: t[Y][i] = 3 s[Y>>1][i] + s[far][i], far = (Y>>1) - 1 for even Y and (Y>>1) + 1 for odd Y;
                    out[Y][2i] = (3 t[Y][i] + t[Y][i-1] + 8) >> 4, out[Y][2i+1] = (3 t[Y][i] + t[Y][i+1] + 7) >> 4
  colour       R = clamp(Y + ((91881 (Cr-128) + 32768) >> 16)), B = clamp(Y + ((116130 (Cb-128) + 32768) >> 16)),
               G = clamp(Y + ((-22554 (Cb-128) - 46802 (Cr-128) + 32768) >> 16));  grayscale: R = G = B = Y
reconstruct(frame, idct="fp64") swaps the inverse DCT for T.81 A.3.3 in float64, rounded to nearest — the accuracy checks' variant."""
import math
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
MAX_SIDE = 65500
MAX_COEFFICIENTS = 1 << 29                                   # int16 values: 1 GiB (178 Mpixel at 4:4:4, 357 Mpixel at 4:2:0)
F_MIN, F_MAX = -2048, 2047
IDCT_BITS, COL_SHIFT, ROW_SHIFT = 13, 9, 17
IDCT_T = np.array([[int(round(2 ** IDCT_BITS * (math.sqrt(0.5) if u == 0 else 1.0) / 2 * math.cos((2 * x + 1) * u * math.pi / 16)))
                    for x in range(8)] for u in range(8)], np.int64)         # [u][x]


class Frame:
    """width, height, ncomp, hs[c], vs[c], quant[c] (uint16[64], natural order), bw[c], bh[c] (blocks per row / column, whole MCUs),
    offset[c] (into coef, in values; multiples of 8 = 16 bytes), coef (int16: component-major, block-row-major, 64 natural-order values per block)"""


def _i32(x):
    assert np.all(x >= -2 ** 31) and np.all(x <= 2 ** 31 - 1), "int32 overflow in the definition"
    return x


class _Huff:
    def __init__(self, counts, symbols):
        self.mincode, self.maxcode, self.valptr, self.symbols = [0] * 17, [-1] * 17, [0] * 17, symbols
        code = k = 0
        for length in range(1, 17):
            self.valptr[length], self.mincode[length] = k, code
            code += counts[length - 1]
            k += counts[length - 1]
            if code > (1 << length):
                raise ValueError("a Huffman table is over-subscribed (its counts overrun the code space)")
            self.maxcode[length] = code - 1 if counts[length - 1] else -1
            code <<= 1


class _Bits:
    """entropy-coded bytes, FF00 unstuffed; past a marker or the end, zero bits are handed out and counted: using one is an error"""
    def __init__(self, data, pos):
        self.d, self.pos, self.acc, self.n, self.fake = data, pos, 0, 0, 0

    def _fill(self):
        while self.n <= 24:
            b = 0
            if self.pos < len(self.d) and self.d[self.pos] != 0xFF:
                b = self.d[self.pos]
                self.pos += 1
            elif self.pos + 1 < len(self.d) and self.d[self.pos + 1] == 0:
                b = 0xFF
                self.pos += 2
            else:
                self.fake += 8
            self.acc = ((self.acc << 8) | b) & 0xFFFFFFFFFFFF
            self.n += 8

    def get(self, k):
        if k == 0:
            return 0
        if self.n < k:
            self._fill()
        self.n -= k
        if self.n < self.fake:
            raise ValueError("truncated scan: the entropy-coded data ends before the last block")
        return (self.acc >> self.n) & ((1 << k) - 1)

    def symbol(self, h):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.get(1)
            if h.maxcode[length] >= 0 and h.mincode[length] <= code <= h.maxcode[length]:
                return h.symbols[h.valptr[length] + code - h.mincode[length]]
        raise ValueError("a Huffman code that is not in the table")

    def restart(self, expect):
        real = self.n - self.fake
        if real < 0 or real // 8:
            raise ValueError("missing or wrong restart marker (data where RST%d belongs)" % expect)
        self.acc = self.n = self.fake = 0
        while self.pos + 1 < len(self.d) and self.d[self.pos] == 0xFF and self.d[self.pos + 1] == 0xFF:
            self.pos += 1
        if not (self.pos + 1 < len(self.d) and self.d[self.pos] == 0xFF and self.d[self.pos + 1] == 0xD0 + expect):
            raise ValueError("missing or wrong restart marker (RST%d expected)" % expect)
        self.pos += 2

    def finish(self):
        real = self.n - self.fake
        if real < 0 or real // 8:
            raise ValueError("bytes after the last block of the scan where a marker belongs")
        return self.pos


def _extend(v, t):
    return v - (1 << t) + 1 if t and v < (1 << (t - 1)) else v


def decode_coefficients(data):
    data = bytes(data)
    if len(data) < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise ValueError("not a JPEG file (no SOI marker)")
    pos = 2
    qt, dc, ac = {}, {}, {}
    sof = None
    restart_interval = 0
    adobe_transform = None
    f = None
    while True:
        if pos >= len(data):
            raise ValueError("truncated: the file ends before " + ("the EOI marker" if f else "a scan"))
        if data[pos] != 0xFF:
            raise ValueError("a marker is expected at byte %d" % pos)
        while pos < len(data) and data[pos] == 0xFF:
            pos += 1
        if pos >= len(data):
            raise ValueError("truncated: the file ends inside a marker")
        m = data[pos]
        pos += 1
        if m == 0xD9:
            if f is None:
                raise ValueError("no scan before the EOI marker")
            return f
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0x00:
            raise ValueError("a marker is expected at byte %d" % (pos - 2))
        if pos + 2 > len(data):
            raise ValueError("truncated: the file ends inside a segment length")
        L = (data[pos] << 8) | data[pos + 1]
        if L < 2 or L > len(data) - pos:
            raise ValueError("segment length %d of marker FF%02X overruns the file (%d bytes left)" % (L, m, len(data) - pos))
        seg = data[pos + 2:pos + L]
        pos += L
        if f is not None:
            if m == 0xDA:
                raise ValueError("multi-scan sequential JPEG: a second scan")
            continue
        if m in (0xC0, 0xC1):
            if sof is not None:
                raise ValueError("a second frame header")
            if len(seg) < 6:
                raise ValueError("truncated frame header")
            if seg[0] != 8:
                raise ValueError("%d-bit JPEG (12-bit is not decoded); only 8-bit" % seg[0])
            h, w, n = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if w == 0 or h == 0 or w > MAX_SIDE or h > MAX_SIDE:
                raise ValueError("image size %dx%d (a side of 0 or above 65500)" % (w, h))
            if n not in (1, 3):
                raise ValueError("%d components (4 = CMYK / YCCK); only grayscale and YCbCr" % n)
            if len(seg) != 6 + 3 * n:
                raise ValueError("frame header length does not match its component count")
            comps = [(seg[6 + 3 * k], seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15, seg[8 + 3 * k]) for k in range(n)]
            for (_, hs, vs, tq) in comps:
                if tq > 3 or not 1 <= hs <= 4 or not 1 <= vs <= 4:
                    raise ValueError("bad sampling factors or quantiser table id in the frame header")
            if n == 3:
                if (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
                    raise ValueError("sampling factors %s; only luma 1x1, 2x1, 2x2 with chroma 1x1" % " ".join("%dx%d" % (c[1], c[2]) for c in comps))
            else:
                comps = [(comps[0][0], 1, 1, comps[0][3])]
            sof = (w, h, comps)
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            kind = {0xC2: "progressive", 0xC3: "lossless", 0xC5: "hierarchical", 0xC6: "hierarchical progressive", 0xC7: "lossless"}.get(m, "arithmetic-coded")
            raise ValueError(kind + " JPEG (SOF%d)" % (m - 0xC0))
        elif m == 0xCC:
            raise ValueError("arithmetic-coded JPEG (DAC)")
        elif m == 0xDB:
            at = 0
            while at < len(seg):
                pq, tq = seg[at] >> 4, seg[at] & 15
                need = 128 if pq == 1 else 64
                if pq > 1 or tq > 3 or at + 1 + need > len(seg):
                    raise ValueError("malformed DQT segment")
                tab = np.zeros(64, np.uint16)
                for k in range(64):
                    tab[ZIGZAG[k]] = (seg[at + 1 + 2 * k] << 8) | seg[at + 2 + 2 * k] if pq else seg[at + 1 + k]
                qt[tq] = tab
                at += 1 + need
        elif m == 0xC4:
            at = 0
            while at < len(seg):
                if at + 17 > len(seg):
                    raise ValueError("malformed DHT segment")
                tc, th = seg[at] >> 4, seg[at] & 15
                counts = list(seg[at + 1:at + 17])
                total = sum(counts)
                if tc > 1 or th > 3:
                    raise ValueError("malformed DHT segment")
                if total > 256 or at + 17 + total > len(seg):
                    raise ValueError("a Huffman table whose counts overrun its segment")
                (ac if tc else dc)[th] = _Huff(counts, list(seg[at + 17:at + 17 + total]))
                at += 17 + total
        elif m == 0xDD:
            if len(seg) != 2:
                raise ValueError("malformed DRI segment")
            restart_interval = (seg[0] << 8) | seg[1]
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                adobe_transform = seg[11]
        elif m == 0xDC:
            raise ValueError("DNL segment (image height defined after the scan)")
        elif m == 0xDA:
            if sof is None:
                raise ValueError("a scan before the frame header")
            w, h, comps = sof
            n = len(comps)
            if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
                raise ValueError("malformed scan header")
            if seg[0] != n:
                raise ValueError("multi-scan sequential JPEG: a scan of %d of the %d components" % (seg[0], n))
            if n == 3 and adobe_transform == 0:
                raise ValueError("RGB JPEG (Adobe transform 0); only grayscale and YCbCr")
            tabs = []
            for k in range(n):
                if seg[1 + 2 * k] != comps[k][0]:
                    raise ValueError("the scan's components are not in frame order")
                td, ta = seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15
                if td not in dc or ta not in ac:
                    raise ValueError("missing Huffman table (DC %d / AC %d)" % (td, ta))
                if comps[k][3] not in qt:
                    raise ValueError("missing quantiser table %d" % comps[k][3])
                tabs.append((dc[td], ac[ta]))
            if seg[1 + 2 * n] != 0 or seg[2 + 2 * n] != 63 or seg[3 + 2 * n] != 0:
                raise ValueError("progressive scan parameters in a sequential JPEG")
            f = Frame()
            f.width, f.height, f.ncomp = w, h, n
            f.hs, f.vs = [c[1] for c in comps], [c[2] for c in comps]
            hmax, vmax = max(f.hs), max(f.vs)
            mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
            f.bw, f.bh = [mx * c[1] for c in comps], [my * c[2] for c in comps]
            f.quant = [qt[c[3]].copy() for c in comps]
            f.offset, total = [], 0
            for k in range(n):
                f.offset.append(total)
                total += f.bw[k] * f.bh[k] * 64
            if total > MAX_COEFFICIENTS:
                raise ValueError("image too large: %d coefficients (the cap is 2^29)" % total)
            if total // 64 > 4 * (len(data) - pos):
                raise ValueError("truncated scan: %d bytes cannot hold %d blocks" % (len(data) - pos, total // 64))
            f.coef = np.zeros(total, np.int16)
            bits = _Bits(data, pos)
            pred = [0] * n
            count = 0
            for mcu in range(mx * my):
                if restart_interval and mcu and mcu % restart_interval == 0:
                    bits.restart(count & 7)
                    count += 1
                    pred = [0] * n
                my_, mx_ = divmod(mcu, mx)
                for k in range(n):
                    for by in range(f.vs[k]):
                        for bx in range(f.hs[k]):
                            base = f.offset[k] + ((my_ * f.vs[k] + by) * f.bw[k] + mx_ * f.hs[k] + bx) * 64
                            t = bits.symbol(tabs[k][0])
                            if t > 15:
                                raise ValueError("bad DC size category")
                            pred[k] += _extend(bits.get(t), t)
                            if not -32768 <= pred[k] <= 32767:
                                raise ValueError("DC coefficient out of the 16-bit range")
                            f.coef[base] = pred[k]
                            i = 1
                            while i < 64:
                                rs = bits.symbol(tabs[k][1])
                                r, s = rs >> 4, rs & 15
                                if s == 0:
                                    if r == 15:
                                        i += 16
                                        if i > 64:
                                            raise ValueError("a zero run past coefficient 63")
                                        continue
                                    if r == 0:
                                        break
                                    raise ValueError("an end-of-band run in a sequential scan")
                                i += r
                                if i > 63:
                                    raise ValueError("a zero run past coefficient 63")
                                f.coef[base + ZIGZAG[i]] = _extend(bits.get(s), s)
                                i += 1
            pos = bits.finish()
        # every other segment (APPn, COM, ...) is skipped


def dequantise(frame, c):
    """-> int64 [bh][bw][8 v][8 u], clamped; clamped_count(frame) tells whether the clamp bit"""
    n = frame.bw[c] * frame.bh[c]
    co = frame.coef[frame.offset[c]:frame.offset[c] + 64 * n].astype(np.int64).reshape(frame.bh[c], frame.bw[c], 8, 8)
    return np.clip(_i32(co * frame.quant[c].astype(np.int64).reshape(8, 8)), F_MIN, F_MAX)


def clamped_count(frame):
    k = 0
    for c in range(frame.ncomp):
        n = frame.bw[c] * frame.bh[c]
        raw = frame.coef[frame.offset[c]:frame.offset[c] + 64 * n].astype(np.int64).reshape(-1, 64) * frame.quant[c].astype(np.int64)
        k += int(((raw < F_MIN) | (raw > F_MAX)).sum())
    return k


def idct_int(F):
    """F int64 [..., 8 v, 8 u] -> samples before the level shift, int64 [..., 8 y, 8 x]"""
    col = _i32(_i32(np.einsum("vy,...vu->...yu", IDCT_T, F)) + (1 << (COL_SHIFT - 1))) >> COL_SHIFT
    assert np.abs(col).max(initial=0) < 1 << 17
    return _i32(_i32(np.einsum("...yu,ux->...yx", col, IDCT_T)) + (1 << (ROW_SHIFT - 1))) >> ROW_SHIFT


def idct_fp64(F):
    """T.81 A.3.3 in float64, rounded to the nearest integer"""
    B = np.array([[(math.sqrt(0.5) if u == 0 else 1.0) / 2 * math.cos((2 * x + 1) * u * math.pi / 16) for x in range(8)] for u in range(8)])
    return np.rint(np.einsum("vy,...vu,ux->...yx", B, F.astype(np.float64), B)).astype(np.int64)


def component_plane(frame, c, idct="int"):
    """-> uint8-valued int64 [bh * 8][bw * 8]"""
    s = (idct_int if idct == "int" else idct_fp64)(dequantise(frame, c))
    s = np.clip(s + 128, 0, 255)
    return s.transpose(0, 2, 1, 3).reshape(frame.bh[c] * 8, frame.bw[c] * 8)


def upsample(plane, hs, vs, W, H):
    """chroma plane (whole blocks) -> [H][W] by the triangle filter; hs, vs are the LUMA sampling factors"""
    if hs == 1 and vs == 1:
        return plane[:H, :W]
    cw, ch = -(-W // hs), -(-H // vs)
    s = plane[:ch, :cw]
    X, Y = np.arange(W), np.arange(H)
    i = X >> 1
    nb = np.clip(np.where(X & 1, i + 1, i - 1), 0, cw - 1)
    if vs == 1:
        return _i32(3 * s[:, i] + s[:, nb] + np.where(X & 1, 2, 1)) >> 2
    j = Y >> 1
    far = np.clip(np.where(Y & 1, j + 1, j - 1), 0, ch - 1)
    t = 3 * s[j, :] + s[far, :]
    return _i32(3 * t[:, i] + t[:, nb] + np.where(X & 1, 7, 8)) >> 4


def reconstruct(frame, idct="int"):
    W, H = frame.width, frame.height
    y = component_plane(frame, 0, idct)[:H, :W]
    if frame.ncomp == 1:
        return np.stack([y, y, y]).astype(np.uint8)
    cb = upsample(component_plane(frame, 1, idct), frame.hs[0], frame.vs[0], W, H) - 128
    cr = upsample(component_plane(frame, 2, idct), frame.hs[0], frame.vs[0], W, H) - 128
    r = y + (_i32(91881 * cr + 32768) >> 16)
    g = y + (_i32(-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + (_i32(116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b]), 0, 255).astype(np.uint8)


def decode(data, idct="int"):
    return reconstruct(decode_coefficients(data), idct)


def synthetic_frame(W, H, hs, vs, ncomp=3, seed=0, coef=None, quant=None):
    """a Frame that no file produced: random coefficients (or the constant `coef`) and quantisers (or the constant `quant`)"""
    r = np.random.default_rng(seed)
    f = Frame()
    f.width, f.height, f.ncomp = W, H, ncomp
    f.hs, f.vs = [hs, 1, 1][:ncomp], [vs, 1, 1][:ncomp]
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    f.bw, f.bh = [mx * h for h in f.hs], [my * v for v in f.vs]
    f.offset, total = [], 0
    for k in range(ncomp):
        f.offset.append(total)
        total += f.bw[k] * f.bh[k] * 64
    if coef is None:
        f.coef = (r.integers(-40, 41, total) * (r.random(total) < 0.25)).astype(np.int16)
        f.coef[::64] = r.integers(-60, 61, total // 64)
    else:
        f.coef = np.asarray(coef, np.int16) if np.ndim(coef) else np.full(total, coef, np.int16)
    f.quant = [np.full(64, quant, np.uint16) if quant is not None else r.integers(1, 24, 64).astype(np.uint16) for _ in range(ncomp)]
    return f
