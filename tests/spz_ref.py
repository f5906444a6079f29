"""numpy restatement of the .spz export (include/dvs_export.h: dvs_pack_spz / dvs_unpack_spz, gsply::write_spz) — TEST INFRASTRUCTURE, not
product code: the yardstick the HIP kernels are compared against bit for bit. Written from the definition of the format, version 3
(DIVSHOT external/spz/src/load-spz.cc: packGaussians with every flip 1, packQuaternionSmallestThree, quantizeSH, unpackGaussians,
unpackQuaternionSmallestThree, serializePackedGaussians; the call in external/tinygsplat/tiny_gsplat.cpp:1232-1272), not from the kernels.
Every operation is float32 in the stated order. The sigmoid is the exception: it is taken in float64, as in compressed_ply_ref, which is
why the alpha byte alone carries the one-step allowance of alpha_slack. Where the reference leaves a case undefined (NaN, values that
are not finite, a degenerate quaternion) the rule of the header is restated."""
import gzip
import struct
import numpy as np
from compressed_ply_ref import alpha_slack, sigmoid64, random_model as _random_geometry          # noqa: F401 (alpha_slack: re-exported)

f32 = np.float32
SECTIONS = ("positions", "alphas", "colors", "scales", "rotations", "sh")
DIM = (0, 3, 8, 15)                                                          # SH coefficients per channel above band 0, by degree
MAGIC = 0x5053474E
SQRT1_2 = f32(0.70710678)
COLOR_SCALE = f32(0.15)


def section_bytes(n, degree):
    return [9 * n, n, 3 * n, 3 * n, 4 * n, 3 * DIM[degree] * n]


def layout(n, degree):
    """(off[6], bytes[6], total) of dvs_spz_layout_for: every section on a 16-byte boundary."""
    off, o = [], 0
    size = section_bytes(n, degree)
    for b in size:
        off.append(o)
        o = (o + b + 15) // 16 * 16
    return off, size, o


def _model(m):
    g = lambda k, w: np.ascontiguousarray(np.asarray(m[k], f32).reshape(-1, w))
    return g("pos", 3), g("sh0", 3), g("shN", 45), g("opacity", 1)[:, 0], g("scale", 3), g("rot", 4)


def round_half_away(x):
    """std::round in float32 (x - trunc(x) is exact)."""
    x = np.asarray(x, f32)
    t = np.trunc(x)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x - t) >= f32(0.5), t + np.copysign(f32(1), x), t).astype(f32)


def to_u8(v):
    """toUint8: (uint8)clamp(round(v), 0, 255); NaN -> 0."""
    r = round_half_away(v)
    r = np.where(np.isnan(r), f32(0), r)
    return np.clip(r, 0, 255).astype(np.uint8)


def pack_positions(pos):
    p = np.asarray(pos, f32).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        f = round_half_away((p * f32(4096.0)).astype(f32))
    f = np.clip(np.where(np.isfinite(p), f, f32(0)), f32(-8388608.0), f32(8388607.0))       # saturated; a p that is not finite -> 0
    v = f.astype(np.int32).astype(np.uint32) & np.uint32(0xFFFFFF)
    return np.stack([v & 255, (v >> 8) & 255, (v >> 16) & 255], axis=1).astype(np.uint8).reshape(-1)


def pack_alphas(opacity):
    o = np.asarray(opacity, f32).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        x = sigmoid64(o) * 255.0
        r = np.where(np.isnan(x), 0.0, np.floor(x + 0.5))                    # (x >= 0: round half away = floor(x + 0.5)); a NaN logit -> 0
    return np.clip(r, 0, 255).astype(np.uint8)


def pack_colors(sh0):
    c = np.asarray(sh0, f32).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        return to_u8((c * f32(COLOR_SCALE * f32(255.0))).astype(f32) + f32(f32(0.5) * f32(255.0)))


def pack_scales(scale):
    s = np.asarray(scale, f32).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        return to_u8(((s + f32(10.0)).astype(f32) * f32(16.0)).astype(f32))


def format_quat(rot):
    """The repository's (w, x, y, z) as the format's normalised (x, y, z, w): divided by sqrt(((x^2 + y^2) + z^2) + w^2); a squared norm
    of 0 or not finite gives (0, 0, 0, 1)."""
    r = np.asarray(rot, f32).reshape(-1, 4)
    q = np.ascontiguousarray(r[:, [1, 2, 3, 0]])
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ss = (((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]).astype(f32) + q[:, 2] * q[:, 2]).astype(f32) + q[:, 3] * q[:, 3]).astype(f32)
        bad = ~(ss > 0) | ~np.isfinite(ss)
        q = (q / np.sqrt(ss, dtype=f32)[:, None]).astype(f32)
    q[bad] = (0, 0, 0, 1)
    return q


def pack_rotations(rot):
    q = format_quat(rot)
    n = len(q)
    a = np.abs(q)
    largest = np.argmax(a, axis=1)                                           # the first index of the strictly greatest magnitude
    negate = q[np.arange(n), largest] < 0
    mag = np.minimum(((f32(511.0) * (a / SQRT1_2).astype(f32)).astype(f32) + f32(0.5)).astype(f32).astype(np.uint32), np.uint32(511))
    negbit = ((q < 0) ^ negate[:, None]).astype(np.uint32)
    comp = largest.astype(np.uint32)
    for k in range(4):
        m = largest != k
        comp[m] = (comp[m] << np.uint32(10)) | (negbit[m, k] << np.uint32(9)) | mag[m, k]
    return np.stack([comp & 255, (comp >> 8) & 255, (comp >> 16) & 255, comp >> 24], axis=1).astype(np.uint8).reshape(-1)


def pack_sh(shN, degree):
    """[n][3 dim] bytes: element j * 3 + c of a splat's 45 higher-order floats -> byte j * 3 + c; bucket 8 for the first 9, 16 after."""
    x = np.asarray(shN, f32).reshape(-1, 45)[:, :3 * DIM[degree]]
    with np.errstate(invalid="ignore", over="ignore"):
        r = round_half_away((x * f32(128.0)).astype(f32))
    r = np.clip(np.where(np.isnan(r), f32(0), r), f32(-512.0), f32(512.0))
    q = r.astype(np.int64) + 128
    b = np.where(np.arange(x.shape[1]) < 9, 8, 16)[None, :]
    t = q + b // 2
    t = np.sign(t) * (np.abs(t) // b) * b                                    # C integer division truncates towards zero
    return np.clip(t, 0, 255).astype(np.uint8).reshape(-1)


def pack(model, degree=3):
    """dict section -> uint8 array, in the order of SECTIONS."""
    pos, sh0, shN, opa, scale, rot = _model(model)
    return {"positions": pack_positions(pos), "alphas": pack_alphas(opa), "colors": pack_colors(sh0), "scales": pack_scales(scale),
            "rotations": pack_rotations(rot), "sh": pack_sh(shN, degree)}


# ---- the loader's side: unpackGaussians -----------------------------------------------------------------------------------------
def unpack(sec, degree=3):
    """dict of pos [n][3], sh0 [n][3], shN [n][45] (0 above the degree), opacity [n] (logit; -inf / +inf for the bytes 0 / 255),
    scale [n][3], rot [n][4] as (w, x, y, z), and `largest` [n] (the format's index of the reconstructed component: 3 = w)."""
    g = lambda k: np.asarray(sec[k], np.uint8).reshape(-1)
    n = len(g("alphas"))
    p = g("positions").reshape(-1, 3).astype(np.uint32)
    v = (p[:, 0] | p[:, 1] << np.uint32(8) | p[:, 2] << np.uint32(16)).astype(np.int64)
    v = np.where(v & 0x800000, v - (1 << 24), v)
    out = {"pos": (v.astype(f32) * f32(1.0 / 4096.0)).astype(f32).reshape(n, 3)}
    out["scale"] = ((g("scales").astype(f32) / f32(16.0)).astype(f32) - f32(10.0)).astype(f32).reshape(n, 3)
    a = (g("alphas").astype(f32) / f32(255.0)).astype(f32)
    with np.errstate(divide="ignore"):
        out["opacity"] = np.log((a / (f32(1.0) - a).astype(f32)).astype(f32).astype(np.float64)).astype(f32)
    out["sh0"] = ((((g("colors").astype(f32) / f32(255.0)).astype(f32) - f32(0.5)).astype(f32)) / COLOR_SCALE).astype(f32).reshape(n, 3)
    shN = np.zeros((n, 45), f32)
    shN[:, :3 * DIM[degree]] = ((g("sh").astype(f32) - f32(128.0)).astype(f32) / f32(128.0)).astype(f32).reshape(n, 3 * DIM[degree])
    out["shN"] = shN
    r = g("rotations").reshape(n, 4).astype(np.uint32)
    comp = r[:, 0] | r[:, 1] << np.uint32(8) | r[:, 2] << np.uint32(16) | r[:, 3] << np.uint32(24)
    largest = (comp >> np.uint32(30)).astype(np.int64)
    q = np.zeros((n, 4), f32)
    total = np.zeros(n, f32)
    for k in (3, 2, 1, 0):
        m = largest != k
        val = ((SQRT1_2 * (comp[m] & np.uint32(511)).astype(f32)).astype(f32) / f32(511.0)).astype(f32)
        val = np.where((comp[m] >> np.uint32(9)) & np.uint32(1), -val, val).astype(f32)
        q[m, k] = val
        total[m] = (total[m] + (val * val).astype(f32)).astype(f32)
        comp[m] = comp[m] >> np.uint32(10)
    q[np.arange(n), largest] = np.sqrt((f32(1.0) - total).astype(f32), dtype=f32)
    out["rot"] = np.ascontiguousarray(q[:, [3, 0, 1, 2]])
    out["largest"] = largest
    return out


# ---- the file -----------------------------------------------------------------------------------------------------------------------
def header(n, degree, antialiased=False):
    return struct.pack("<IIIBBBB", MAGIC, 3, n, degree, 12, 1 if antialiased else 0, 0)


def parse_spz(raw):
    """(n, degree, antialiased, sections) of the gunzipped bytes of a file; asserts the header and the exact size."""
    magic, version, n, degree, frac, flags, reserved = struct.unpack("<IIIBBBB", raw[:16])
    assert (magic, version, frac, reserved) == (MAGIC, 3, 12, 0) and degree <= 3 and flags in (0, 1), (magic, version, degree, frac, flags, reserved)
    size = section_bytes(n, degree)
    assert len(raw) == 16 + sum(size), (len(raw), 16 + sum(size))
    sec, at = {}, 16
    for name, b in zip(SECTIONS, size):
        sec[name] = np.frombuffer(raw, np.uint8, b, at).copy()
        at += b
    return n, degree, bool(flags & 1), sec


def read_spz(path):
    with gzip.open(path, "rb") as f:
        return parse_spz(f.read())


# ---- inputs the CPU and the GPU tests share -----------------------------------------------------------------------------------------
def random_model(n, seed=0, pos_scale=4.0):
    """compressed_ply_ref.random_model plus the 45 higher-order SH floats, uniform in [-1.2, 1.2] (past both ends of the byte range)."""
    m = _random_geometry(n, seed, pos_scale)
    m["shN"] = np.random.default_rng(seed + 7919).uniform(-1.2, 1.2, (n, 45)).astype(f32)
    return m


EDGE_CASES = ("nan", "pos_inf", "neg_inf", "zero_quat", "far_positions", "logits_pm30", "equal_quat")
FIELDS = ("pos", "sh0", "shN", "opacity", "scale", "rot")


def edge_model(name, n=200):
    """random_model(n) with the edge the name says (n = 200: three full tiles and a partial one)."""
    m = random_model(n, seed=500 + EDGE_CASES.index(name))
    special = {"nan": np.nan, "pos_inf": np.inf, "neg_inf": -np.inf}
    if name in special:                                                      # in each array, on different splats, every 7th from k on
        for k, field in enumerate(FIELDS):
            a = m[field].reshape(n, -1)
            a[k::7, k % a.shape[1]] = special[name]
    elif name == "zero_quat":
        m["rot"][::3] = 0.0
        m["rot"][1] = (1e-30, 0, 0, 0)                                       # the squared norm underflows to 0
        m["rot"][2] = (3e19, 3e19, 0, 0)                                     # the squared norm overflows
    elif name == "far_positions":                                            # |pos| >= 2048: saturates
        m["pos"][:] = (np.sign(m["pos"]) * np.random.default_rng(3).uniform(2048, 1e6, (n, 3))).astype(f32)
        m["pos"][0] = (2048.0, -2048.0, 2047.99987793)                       # the ends: 2^23 saturates, -2^23 fits, 2^23 - 0.5 rounds up and saturates
        m["pos"][1] = (3e38, -3e38, 1e30)                                    # p * 4096 overflows: finite p, saturated
    elif name == "logits_pm30":
        m["opacity"][:] = np.where(np.arange(n) % 2 == 0, 30.0, -30.0).astype(f32)
    elif name == "equal_quat":
        pats = np.array([(0.5, 0.5, 0.5, 0.5), (-0.5, -0.5, -0.5, -0.5), (0.5, -0.5, 0.5, -0.5), (-3, 3, 3, 3), (0, 0.7, -0.7, 0), (0, 0, -2, -2)], f32)
        m["rot"][:] = pats[np.arange(n) % len(pats)]
    else:
        raise KeyError(name)
    return m
