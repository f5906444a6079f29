"""numpy restatement of the compact model exports (include/dvs_export.h) — TEST INFRASTRUCTURE, not product code: the yardstick the HIP
packers are compared against bit for bit. Written from the definitions of the formats (DIVSHOT external/tinygsplat: packUnorm / pack8888 /
packColor / SplatChunk::pack and unpack, tiny_gsplat.hpp:342-534; the Morton interleave and the file layout, tiny_gsplat.cpp:293-396; the
32-byte record, tiny_gsplat.cpp:243-291), not from the kernels. Every operation is float32 in an explicit order; the sigmoid is the
exception, it is taken in float64 (which is why the alpha byte alone carries a documented one-step allowance, see alpha_slack)."""
import numpy as np

f32 = np.float32
C0 = f32(0.28209479177387814)
CHUNK = 256


def _model(m):
    g = lambda k, w: np.ascontiguousarray(np.asarray(m[k], f32).reshape(-1, w))
    return g("pos", 3), g("sh0", 3), g("opacity", 1)[:, 0], g("scale", 3), g("rot", 4)


# ---- (a) - (c): Morton order ------------------------------------------------------------------------------------------------------
def morton_keys(pos):
    """30-bit keys: q_a = (uint32)(rel_a * 1023.0f), rel_a = ext_a < 1e-5f ? 0 : (p_a - min_a) / ext_a; bit i of q_x / q_y / q_z -> key bit
    3i / 3i + 1 / 3i + 2."""
    pos = np.asarray(pos, f32).reshape(-1, 3)
    mn, mx = pos.min(axis=0), pos.max(axis=0)
    ext = (mx - mn).astype(f32)
    key = np.zeros(len(pos), np.uint32)
    for a in range(3):
        if ext[a] < f32(1e-5):
            rel = np.zeros(len(pos), f32)
        else:
            rel = ((pos[:, a] - mn[a]).astype(f32) / ext[a]).astype(f32)
        q = (rel * f32(1023.0)).astype(f32).astype(np.uint32)                # truncation; rel is in [0, 1]
        assert q.max(initial=0) <= 1023
        for i in range(10):
            key |= ((q >> np.uint32(i)) & np.uint32(1)) << np.uint32(3 * i + a)
    return key


def morton_order(pos):
    """order[j] = model index of output vertex j: stable sort of the keys, ties in index order."""
    return np.argsort(morton_keys(pos), kind="stable").astype(np.uint32)


# ---- (d): the packed words ---------------------------------------------------------------------------------------------------------
def pack_unorm(v, bits):
    """clamp(floor((double)(v * t) + 0.5), 0, t), t = 2^bits - 1, the product in float32 (tiny_gsplat.hpp:342-346)."""
    t = (1 << bits) - 1
    p = (np.asarray(v, f32) * f32(t)).astype(f32)
    return np.clip(np.floor(p.astype(np.float64) + 0.5), 0, t).astype(np.uint32)


def pack111011(x, y, z):
    return pack_unorm(x, 11) << np.uint32(21) | pack_unorm(y, 10) << np.uint32(11) | pack_unorm(z, 11)


def _norm(x, mn, mx):
    e = f32(mx - mn)
    if e < f32(0.00001):
        return np.zeros_like(x)
    return ((x - mn).astype(f32) / e).astype(f32)


def normalized_quat(rot):
    """q / sqrt(((r0^2 + r1^2) + r2^2) + r3^2); a squared norm of 0 or not finite gives (1, 0, 0, 0)."""
    r = np.asarray(rot, f32).reshape(-1, 4)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ss = (((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]).astype(f32) + r[:, 2] * r[:, 2]).astype(f32) + r[:, 3] * r[:, 3]).astype(f32)
        bad = ~(ss > 0) | ~np.isfinite(ss)
        q = (r / np.sqrt(ss, dtype=f32)[:, None]).astype(f32)
    q[bad] = (1, 0, 0, 0)
    return q


def pack_rotation(rot):
    q = normalized_quat(rot)
    n = len(q)
    largest = np.argmax(np.abs(q), axis=1)                                   # the first index of the greatest magnitude
    neg = q[np.arange(n), largest] < 0
    q[neg] = -q[neg]
    pu = pack_unorm((q * f32(0.70710678)).astype(f32) + f32(0.5), 10)
    res = largest.astype(np.uint32)
    for k in range(4):
        m = largest != k
        res[m] = (res[m] << np.uint32(10)) | pu[m, k]
    return res


def sigmoid64(opacity):
    return 1.0 / (1.0 + np.exp(-np.asarray(opacity, np.float64)))


def alpha_slack(opacity):
    """Where the alpha byte of packed_color may differ by one from a float32 sigmoid: sigmoid * 255 + 0.5 in float64 within 1e-3 of an
    integer (a float32 sigmoid good to a few ulp moves the product by about 1e-4)."""
    x = sigmoid64(opacity) * 255.0 + 0.5
    return np.abs(x - np.round(x)) < 1e-3


def pack_color(sh0, opacity):
    c = pack_unorm((np.asarray(sh0, f32) * C0).astype(f32) + f32(0.5), 8)
    a = np.clip(np.floor(sigmoid64(opacity) * 255.0 + 0.5), 0, 255).astype(np.uint32)
    return c[:, 0] << np.uint32(24) | c[:, 1] << np.uint32(16) | c[:, 2] << np.uint32(8) | a


def encode_in_order(model, order):
    """(chunks [ceil(n/256)][12], verts [n][4]) for a given vertex order; verts columns are the file's vertex properties:
    packed_position, packed_rotation, packed_scale, packed_color."""
    pos, sh0, opa, scale, rot = _model(model)
    order = np.asarray(order, np.int64)
    n = len(order)
    nch = (n + CHUNK - 1) // CHUNK
    p, s = pos[order], scale[order]
    chunks = np.zeros((nch, 12), f32)
    verts = np.zeros((n, 4), np.uint32)
    for c in range(nch):
        sl = slice(c * CHUNK, min(n, (c + 1) * CHUNK))
        pc, sc = p[sl], s[sl]
        pmin, pmax, smin, smax = pc.min(axis=0), pc.max(axis=0), sc.min(axis=0), sc.max(axis=0)      # over the chunk's own members
        chunks[c] = np.concatenate([pmin, pmax, smin, smax])
        verts[sl, 0] = pack111011(*[_norm(pc[:, a], pmin[a], pmax[a]) for a in range(3)])
        verts[sl, 2] = pack111011(*[_norm(sc[:, a], smin[a], smax[a]) for a in range(3)])
    verts[:, 1] = pack_rotation(rot[order])
    verts[:, 3] = pack_color(sh0[order], opa[order])
    return chunks, verts


def encode(model):
    """(chunks, verts, order) of dvs_pack_compressed."""
    order = morton_order(_model(model)[0])
    chunks, verts = encode_in_order(model, order)
    return chunks, verts, order


# ---- the loader's side: SplatChunk::unpack / unpackColor (tiny_gsplat.hpp:364-386, 470-533) ----------------------------------------
def _unorm(p, bits):
    mx = (1 << bits) - 1
    return ((np.asarray(p, np.uint32) & np.uint32(mx)).astype(f32) / f32(mx)).astype(f32)


def decode(chunks, verts):
    """dict of pos, scale, rot, sh0, opacity (logit; +-inf at the byte's ends) and alpha (the byte / 255), in the file's vertex order."""
    chunks = np.asarray(chunks, f32).reshape(-1, 12)
    verts = np.asarray(verts, np.uint32).reshape(-1, 4)
    n = len(verts)
    ci = np.arange(n) // CHUNK
    out = {}
    for name, col, base in (("pos", 0, 0), ("scale", 2, 6)):
        w = verts[:, col]
        u = np.stack([_unorm(w >> np.uint32(21), 11), _unorm(w >> np.uint32(11), 10), _unorm(w, 11)], axis=1)
        mn, mx = chunks[ci, base:base + 3], chunks[ci, base + 3:base + 6]
        out[name] = (u * (mx - mn).astype(f32) + mn).astype(f32)
    w = verts[:, 1]
    norm = 1.0 / (np.sqrt(2.0) * 0.5)
    abc = np.stack([((_unorm(w >> np.uint32(s), 10).astype(np.float64) - 0.5) * norm).astype(f32) for s in (20, 10, 0)], axis=1)
    with np.errstate(invalid="ignore"):
        m = np.sqrt(f32(1.0) - ((abc[:, 0] * abc[:, 0] + abc[:, 1] * abc[:, 1]).astype(f32) + abc[:, 2] * abc[:, 2]).astype(f32), dtype=f32)
    rot = np.zeros((n, 4), f32)
    largest = (w >> np.uint32(30)).astype(np.int64)
    for k in range(4):
        sel = largest == k
        rot[sel, k] = m[sel]
        rot[np.ix_(sel, [i for i in range(4) if i != k])] = abc[sel]
    out["rot"] = rot
    w = verts[:, 3]
    out["sh0"] = np.stack([((_unorm(w >> np.uint32(s), 8) - f32(0.5)) / C0).astype(f32) for s in (24, 16, 8)], axis=1)
    out["alpha"] = _unorm(w, 8)
    with np.errstate(divide="ignore"):
        out["opacity"] = (-np.log(f32(1.0) / out["alpha"] - f32(1.0))).astype(f32)
    return out


# ---- (e): the 32-byte .splat record -----------------------------------------------------------------------------------------------
def _trunc_u8(v):
    return np.clip(v, 0, 255).astype(np.uint8)                               # (u8) of a clamped value truncates


def encode_splat32(model):
    """uint8 [n][32] in the model's order. Bytes 12-23 hold exp(scale) from float64 (the device's deterministic exp is < 2 ulp from it:
    compare those with a tolerance); byte 27 is the truncated float64 sigmoid * 255 (see splat32_slack)."""
    pos, sh0, opa, scale, rot = _model(model)
    n = len(pos)
    out = np.zeros((n, 32), np.uint8)
    out[:, 0:12] = pos.view(np.uint8).reshape(n, 12)
    out[:, 12:24] = np.exp(scale.astype(np.float64)).astype(f32).view(np.uint8).reshape(n, 12)
    out[:, 24:27] = _trunc_u8(((f32(0.5) + (C0 * sh0).astype(f32)).astype(f32) * f32(255.0)).astype(f32))
    out[:, 27] = _trunc_u8(sigmoid64(opa) * 255.0)
    out[:, 28:32] = _trunc_u8((normalized_quat(rot) * f32(128.0)).astype(f32) + f32(128.0))
    return out


def splat32_slack(model):
    """bool [n][4]: where bytes 24-27 may differ by one step — the value before truncation, taken in float64, within 1e-3 of an integer."""
    _, sh0, opa, _, _ = _model(model)
    x = np.concatenate([(0.5 + float(C0) * sh0.astype(np.float64)) * 255.0, (sigmoid64(opa) * 255.0)[:, None]], axis=1)
    return np.abs(x - np.round(x)) < 1e-3


# ---- the file ---------------------------------------------------------------------------------------------------------------------
CHUNK_PROPS = ("min_x", "min_y", "min_z", "max_x", "max_y", "max_z", "min_scale_x", "min_scale_y", "min_scale_z", "max_scale_x",
               "max_scale_y", "max_scale_z")
VERTEX_PROPS = ("packed_position", "packed_rotation", "packed_scale", "packed_color")


def header(n, antialiased=False):
    """The header of tiny_gsplat.cpp:371-391, byte for byte."""
    h = "ply\nformat binary_little_endian 1.0\ncomment generated by diverseshot\n"
    if antialiased:
        h += "comment splatx.anti_aliasing=1\n"
    h += f"element chunk {(n + CHUNK - 1) // CHUNK}\n" + "".join(f"property float {p}\n" for p in CHUNK_PROPS)
    h += f"element vertex {n}\n" + "".join(f"property uint {p}\n" for p in VERTEX_PROPS) + "end_header\n"
    return h.encode()


def read_compressed_ply(path):
    """(chunks, verts) of a .compressed.ply; the header must be exactly header(n)."""
    blob = open(path, "rb").read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode().split("\n")
    n = int([l for l in lines if l.startswith("element vertex ")][0].split()[-1])
    aa = "comment splatx.anti_aliasing=1" in lines
    assert blob[:end] == header(n, aa), blob[:end]
    nch = (n + CHUNK - 1) // CHUNK
    assert len(blob) == end + 48 * nch + 16 * n
    chunks = np.frombuffer(blob, f32, nch * 12, end).reshape(nch, 12)
    verts = np.frombuffer(blob, np.uint32, n * 4, end + 48 * nch).reshape(n, 4)
    return chunks, verts


def random_model(n, seed=0, pos_scale=4.0):
    """A model with the value ranges of a trained scene: logits uniform in [-6, 6], log-scales in [-7, -1], sh0 in [-2.5, 2.5]."""
    r = np.random.default_rng(seed)
    return {"pos": (r.uniform(-1, 1, (n, 3)) * pos_scale).astype(f32), "sh0": r.uniform(-2.5, 2.5, (n, 3)).astype(f32),
            "opacity": r.uniform(-6, 6, n).astype(f32), "scale": r.uniform(-7, -1, (n, 3)).astype(f32),
            "rot": r.normal(size=(n, 4)).astype(f32)}


# ---- inputs the CPU and the GPU tests share -----------------------------------------------------------------------------------------
EDGE_CASES = ("one_point", "constant_scale", "duplicates", "zero_quat", "negative_largest", "equal_magnitude", "opacity_pm20",
              "sh0_saturated", "pos_1e-3_to_1e3")


def edge_model(name, n=777):
    """random_model(n) with one field replaced by the edge the name says (n = 777: three full chunks and a partial one)."""
    m = random_model(n, seed=100 + EDGE_CASES.index(name))
    r = np.random.default_rng(7)
    if name == "one_point":                                                  # extent < 1e-5 on every axis: all keys equal, order = identity
        m["pos"][:] = (0.25, -3.0, 7.5)
    elif name == "constant_scale":                                           # scale extent 0 in every chunk: norm() takes its zero branch
        m["scale"][:] = (-4.0, -3.5, -5.0)
    elif name == "duplicates":                                               # many exact duplicates of 5 positions: ties, stable order
        pts = m["pos"][:5].copy()
        m["pos"][:] = pts[r.integers(0, 5, n)]
    elif name == "zero_quat":
        m["rot"][::3] = 0.0
        m["rot"][1] = (np.inf, 0, 0, 0)                                      # squared norm not finite
        m["rot"][2] = (1e-30, 0, 0, 0)                                       # squared norm underflows to 0
    elif name == "negative_largest":
        m["rot"] = np.abs(m["rot"])
        k = r.integers(0, 4, n)
        m["rot"][np.arange(n), k] = -(m["rot"].max(axis=1) + 0.5)
    elif name == "equal_magnitude":
        pats = np.array([(0.5, 0.5, 0.5, 0.5), (0.5, -0.5, 0.5, -0.5), (-0.7, 0.7, 0, 0), (0, -0.25, 0.25, 0), (0, 0, -3, -3), (-1, -1, -1, 1)], f32)
        m["rot"][:] = pats[np.arange(n) % len(pats)]
    elif name == "opacity_pm20":
        m["opacity"][:] = np.where(np.arange(n) % 2 == 0, 20.0, -20.0).astype(f32)
    elif name == "sh0_saturated":
        m["sh0"][:] = np.where(r.uniform(size=(n, 3)) < 0.5, -10.0, 10.0).astype(f32)
        m["sh0"][::7] = (-0.5 / float(C0), 0.5 / float(C0), 0.0)            # and the exact ends of the byte range
    elif name == "pos_1e-3_to_1e3":
        m["pos"][:] = (np.sign(r.uniform(-1, 1, (n, 3))) * 10.0 ** r.uniform(-3, 3, (n, 3))).astype(f32)
    else:
        raise KeyError(name)
    return m


def assert_within_format_bounds(model, chunks, verts, order):
    """decode(chunks, verts), un-permuted by `order`, against the model, per chunk, within what the format can hold:
      position, scale   half a quantisation step of the chunk's extent: extent / (2 * 2047) in x and z, extent / (2 * 1023) in y, plus a
                        few float32 ulp of the box (normalise, scale by t, divide by t, un-normalise: <= 8 roundings of values inside the
                        box); an axis whose extent is below the format's 1e-5 guard decodes to the chunk's minimum: error <= extent
      colour            0.5 / 255 / C0 where the byte is not saturated; saturated values decode to the byte's end
      alpha             0.5 / 255 of the float64 sigmoid (+ 1e-6 for a float32 sigmoid on the packing side)
      rotation          the three stored components within d = sqrt(2) / (2 * 1023) of the normalised quaternion, up to sign; the fourth is
                        recomputed as m = sqrt(1 - a^2 - b^2 - c^2): |dm| <= d (6 m + 3 d) / (m_dec + m), 3 d to first order (m >= 1/2 is
                        the largest component) — asserted as 4 d."""
    pos, sh0, opa, scale, rot = _model(model)
    order = np.asarray(order, np.int64)
    chunks = np.asarray(chunks, f32).reshape(-1, 12)
    d = decode(chunks, verts)
    n = len(order)
    ci = np.arange(n) // CHUNK
    eps = float(np.finfo(f32).eps)
    steps = np.array([2047.0, 1023.0, 2047.0])
    for name, src, base in (("pos", pos, 0), ("scale", scale, 6)):
        mn, mx = chunks[ci, base:base + 3].astype(np.float64), chunks[ci, base + 3:base + 6].astype(np.float64)
        ext = (chunks[ci, base + 3:base + 6] - chunks[ci, base:base + 3]).astype(np.float64)
        tol = np.where(ext < 1e-5, ext, ext / (2 * steps)) + 8 * eps * np.maximum(np.abs(mn), np.abs(mx))
        err = np.abs(d[name].astype(np.float64) - src[order].astype(np.float64))
        assert (err <= tol).all(), (name, float((err - tol).max()))
    x = sh0[order].astype(np.float64) * float(C0) + 0.5
    inside = (x >= 0) & (x <= 1)
    err = np.abs(d["sh0"].astype(np.float64) - sh0[order])
    assert (err[inside] <= 0.5 / 255 / float(C0) + 8 * eps * 3).all(), float(err[inside].max())
    ends = np.where(x < 0, f32(-0.5) / C0, f32(0.5) / C0)
    assert np.array_equal(d["sh0"][~inside], ends[~inside].astype(f32))
    assert (np.abs(d["alpha"].astype(np.float64) - sigmoid64(opa[order])) <= 0.5 / 255 + 1e-6).all()
    q = normalized_quat(rot[order]).astype(np.float64)
    largest = (np.asarray(verts, np.uint32).reshape(-1, 4)[:, 1] >> np.uint32(30)).astype(np.int64)
    ql = q[np.arange(n), largest]
    assert (np.abs(ql) >= np.abs(q).max(axis=1) - 4 * eps).all()
    q = q * np.where(ql < 0, -1.0, 1.0)[:, None]
    dq = np.sqrt(2.0) / (2 * 1023) + 4 * eps
    err = np.abs(d["rot"].astype(np.float64) - q)
    stored = np.arange(4)[None, :] != largest[:, None]
    assert (err[stored] <= dq).all(), float(err[stored].max())
    assert (err[~stored] <= 4 * dq).all(), float(err[~stored].max())
