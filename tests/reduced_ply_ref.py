"""numpy restatement of the .reduced.ply export (include/dvs_export.h: dvs_sh_degree_select, dvs_codebooks_build, dvs_pack_reduced,
dvs_unpack_reduced, gsply::write_reduced_ply) — TEST INFRASTRUCTURE, not product code: the yardstick the HIP kernels and the host writer
are compared with. Written from the header's definitions and the container's layout (four per-degree vertex blocks, then the table of
twenty 256-entry codebooks, row = entry), not from anybody's program text.
A model is a dict of float32 arrays: pos [n,3], sh0 [n,3], shN [n,45] (coefficient-major, channel-minor), opacity [n], scale [n,3],
rot [n,4] as (w, x, y, z)."""
import re
import numpy as np

f32, f64 = np.float32, np.float64
BOOKS, ENTRIES = 20, 256
NAMES = ["f_dc"] + [f"f_rest_{j}" for j in range(15)] + ["opacity", "scale", "rot_re", "rot_im"]
FIELDS = ("pos", "sh0", "shN", "opacity", "scale", "rot")
MAX_VALUES = 1 << 25

# the rasterizer's basis constants (csrc/dvs_device.h)
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)


def coeffs(d):
    return (d + 1) * (d + 1) - 1


def stride(d, half):
    return (6 if half else 12) + 3 + 3 * coeffs(d) + 8


# ---- per-splat degree -----------------------------------------------------------------------------------------------------------------
def basis(d):
    """d [..., 3] unit directions -> [..., 16] float64 (entry 0 is the constant band)"""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    b = [np.full_like(x, 0.28209479177387814), -C1 * y, C1 * z, -C1 * x,
         C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy),
         C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy), C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
         C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy), C3[6] * x * (xx - 3 * yy)]
    return np.stack(b, axis=-1)


def degree_errors(pos, shN, cams, D):
    """err [n, 3] in float64: err[:, k] = the most any camera and channel loses when the splat is cut to degree k (0 for k >= D)"""
    pos, shN, cams = np.asarray(pos, f64).reshape(-1, 3), np.asarray(shN, f64).reshape(-1, 15, 3), np.asarray(cams, f64).reshape(-1, 3)
    n = len(pos)
    err = np.zeros((n, 3))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for o in cams:
            v = pos - o
            length = np.sqrt((v * v).sum(1))
            use = (length > 0) & np.isfinite(length)
            b = basis(v / length[:, None])                                   # [n, 16]
            for k in range(min(D, 3)):
                lo, hi = coeffs(k), coeffs(D)                                # coefficients of the bands k < band <= D
                lost = np.abs(np.einsum("nl,nlc->nc", b[:, 1 + lo:1 + hi], shN[:, lo:hi])).max(1)
                lost = np.where(np.isnan(lost), np.inf, lost)                # not finite: exceeds every threshold
                err[:, k] = np.where(use, np.maximum(err[:, k], lost), err[:, k])
    return err


def select_degrees(pos, shN, cams, D, t):
    """-> (degree uint8 [n], undecided bool [n]): undecided = some err_k lies within 1e-4 t + 1e-7 of t"""
    err = degree_errors(pos, shN, cams, D)
    ok = np.concatenate([err[:, :D] <= t, np.ones((len(err), 1), bool)], axis=1)        # err_D = 0
    with np.errstate(invalid="ignore"):
        undecided = (np.abs(err[:, :D] - t) <= 1e-4 * t + 1e-7).any(1)
    return np.argmax(ok, axis=1).astype(np.uint8), undecided


# ---- codebooks ------------------------------------------------------------------------------------------------------------------------
def clean(v):
    """what is clustered: float32, a value that is not finite and -0 count as +0"""
    v = np.array(v, f32).reshape(-1)
    v[~np.isfinite(v)] = 0
    return v + f32(0)                                                        # (-0 + 0 = +0)


def boundaries(c):
    """the 255 boundaries of the centres c, ascending: the cluster of v is #{j : b_j < v}, its position among the SORTED boundaries"""
    c = np.asarray(c, f32).astype(f64)
    return np.sort((c[:-1] + c[1:]) * 0.5)


def ids_for(c, values):
    return np.searchsorted(boundaries(c), clean(values).astype(f64), "left").astype(np.uint8)


def build_codebook(values, max_iters=100):
    """-> (centres float32 [256], iterations run); the header's rules 1-5, independent of the order of `values`"""
    s = np.sort(clean(values))
    m = len(s)
    assert m <= MAX_VALUES and max_iters >= 1
    if m == 0 or np.abs(s).max() == 0:
        return np.zeros(ENTRIES, f32), 0
    e = int(np.frexp(f64(np.abs(s).max()))[1])                               # A = f 2^e with f in [0.5, 1)
    k = np.rint(np.ldexp(s.astype(f64), 36 - e)).astype(np.int64)            # (rint: ties to even)
    prefix = np.concatenate([[0], np.cumsum(k, dtype=np.int64)])
    c = s[((2 * np.arange(ENTRIES, dtype=np.int64) + 1) * m) // 512].copy()
    s64 = s.astype(f64)
    prev, iters = None, 0
    while iters < max_iters:
        ends = np.concatenate([np.searchsorted(s64, boundaries(c), "right"), [m]]).astype(np.int64)
        if prev is not None and np.array_equal(ends, prev):
            break
        starts = np.concatenate([[0], ends[:-1]])
        count = ends - starts
        full = count > 0
        total = prefix[ends] - prefix[starts]
        c[full] = np.ldexp(total[full].astype(f64) / count[full].astype(f64), e - 36).astype(f32)
        prev = ends
        iters += 1
    return c, iters


def cluster_by_count(c, values):
    """the definition itself, without a sort: #{j : b_j < v} (for the tests of ids_for)"""
    c = np.asarray(c, f32).astype(f64)
    b = (c[:-1] + c[1:]) * 0.5
    return (b[None, :] < clean(values).astype(f64)[:, None]).sum(1)


def normalised_rot(rot):
    """(w, x, y, z) / sqrt(((w^2 + x^2) + y^2) + z^2) in float32; a squared norm of 0 or not finite gives (1, 0, 0, 0)"""
    r = np.asarray(rot, f32).reshape(-1, 4)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ss = (((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]).astype(f32) + r[:, 2] * r[:, 2]).astype(f32) + r[:, 3] * r[:, 3]).astype(f32)
        bad = ~(ss > 0) | ~np.isfinite(ss)
        q = (r / np.sqrt(ss, dtype=f32)[:, None]).astype(f32)
    q[bad] = (1, 0, 0, 0)
    return q


def _deg(degrees):
    return np.minimum(np.asarray(degrees, np.uint8).reshape(-1), 3).astype(np.int64)


def value_sets(model, degrees):
    """the twenty value sets, in the file's column order"""
    deg = _deg(degrees)
    shN = np.asarray(model["shN"], f32).reshape(-1, 15, 3)
    q = normalised_rot(model["rot"])
    sets = [np.asarray(model["sh0"], f32).reshape(-1)]
    for j in range(15):
        sets.append(shN[np.array([coeffs(d) for d in range(4)])[deg] > j, j, :].reshape(-1))
    sets += [np.asarray(model["opacity"], f32).reshape(-1), np.asarray(model["scale"], f32).reshape(-1), q[:, 0].copy(), q[:, 1:].reshape(-1)]
    return sets


def build_codebooks(model, degrees, max_iters=100):
    """-> (centres float32 [20, 256], iterations int32 [20])"""
    out = [build_codebook(v, max_iters) for v in value_sets(model, degrees)]
    return np.stack([c for c, _ in out]), np.array([i for _, i in out], np.int32)


# ---- the payload ----------------------------------------------------------------------------------------------------------------------
def to_half(x):
    """float32 -> the bits of the half: round to nearest even, |x| >= 65520 (infinities too) saturates to +-65504, NaN -> 0"""
    x = np.array(x, f32)
    x[np.isnan(x)] = 0
    return np.clip(x, -65504, 65504).astype(np.float16).view(np.uint16)


def layout(counts, half):
    counts = [int(c) for c in counts]
    strides = [stride(d, half) for d in range(4)]
    off = [sum(counts[k] * strides[k] for k in range(d)) for d in range(4)]
    table = off[3] + counts[3] * strides[3]
    return {"count": counts, "off": off, "stride": strides, "table_off": table, "total": table + BOOKS * ENTRIES * 4, "half": int(bool(half))}


def block_order(degrees):
    """model indices in the file's order: degree 0 first, the model's order inside a degree"""
    return np.argsort(_deg(degrees), kind="stable")


def pack(model, degrees, centres, half=False):
    """-> the payload (uint8): what follows end_header"""
    deg = _deg(degrees)
    n = len(deg)
    centres = np.asarray(centres, f32).reshape(BOOKS, ENTRIES)
    L = layout(np.bincount(deg, minlength=4), half)
    out = np.zeros(L["total"], np.uint8)
    pos = np.asarray(model["pos"], f32).reshape(n, 3)
    xyz = to_half(pos).view(np.uint8).reshape(n, 6) if half else pos.view(np.uint8).reshape(n, 12)
    shN = np.asarray(model["shN"], f32).reshape(n, 15, 3)
    q = normalised_rot(model["rot"])
    dc = ids_for(centres[0], model["sh0"]).reshape(n, 3)
    rest = np.stack([ids_for(centres[1 + j], shN[:, j, :]).reshape(n, 3) for j in range(15)], axis=1).reshape(n, 45)
    tail = np.concatenate([ids_for(centres[16], model["opacity"]).reshape(n, 1), ids_for(centres[17], model["scale"]).reshape(n, 3),
                           ids_for(centres[18], q[:, 0]).reshape(n, 1), ids_for(centres[19], q[:, 1:]).reshape(n, 3)], axis=1)
    for d in range(4):
        who = np.nonzero(deg == d)[0]
        rec = np.concatenate([xyz[who], dc[who], rest[who, :3 * coeffs(d)], tail[who]], axis=1)
        assert rec.shape[1] == L["stride"][d]
        out[L["off"][d]:L["off"][d] + rec.size] = rec.reshape(-1)
    out[L["table_off"]:] = np.ascontiguousarray(centres.T).view(np.uint8).reshape(-1)
    return out


def decode(payload, counts, half):
    """what the viewer's loader reconstructs: the splats in block order, coefficients above a splat's degree 0 -> a model + "degree" """
    L = layout(counts, half)
    payload = np.asarray(payload, np.uint8)
    assert len(payload) == L["total"], (len(payload), L["total"])
    table = payload[L["table_off"]:].view(f32).reshape(ENTRIES, BOOKS)
    n = sum(L["count"])
    m = {"pos": np.zeros((n, 3), f32), "sh0": np.zeros((n, 3), f32), "shN": np.zeros((n, 45), f32), "opacity": np.zeros(n, f32),
         "scale": np.zeros((n, 3), f32), "rot": np.zeros((n, 4), f32), "degree": np.zeros(n, np.uint8)}
    at = 0
    for d in range(4):
        cnt, st, xyz = L["count"][d], L["stride"][d], 6 if half else 12
        rec = payload[L["off"][d]:L["off"][d] + cnt * st].reshape(cnt, st)
        sl = slice(at, at + cnt)
        raw = np.ascontiguousarray(rec[:, :xyz])
        m["pos"][sl] = raw.view(np.float16).astype(f32) if half else raw.view(f32)
        m["sh0"][sl] = table[rec[:, xyz:xyz + 3], 0]
        ids = rec[:, xyz + 3:xyz + 3 + 3 * coeffs(d)]
        m["shN"][sl, :3 * coeffs(d)] = table[ids, 1 + np.arange(3 * coeffs(d)) // 3]
        t = rec[:, xyz + 3 + 3 * coeffs(d):]
        m["opacity"][sl] = table[t[:, 0], 16]
        m["scale"][sl] = table[t[:, 1:4], 17]
        m["rot"][sl, 0] = table[t[:, 4], 18]
        m["rot"][sl, 1:] = table[t[:, 5:8], 19]
        m["degree"][sl] = d
        at += cnt
    return m


# ---- the file -------------------------------------------------------------------------------------------------------------------------
def header_lines(counts, half):
    lines = ["ply", "format binary_little_endian 1.0", "comment generated by diverseshot"]
    for d in range(4):
        lines.append(f"element vertex {int(counts[d])}")
        lines += [f"property {'f16' if half else 'float'} {a}" for a in "xyz"]
        lines += [f"property u8 f_dc_{k}" for k in range(3)]
        lines += [f"property u8 f_rest_{k}" for k in range(3 * coeffs(d))]
        lines += ["property u8 opacity"] + [f"property u8 scale_{k}" for k in range(3)] + [f"property u8 rot_{k}" for k in range(4)]
    lines.append(f"element cook_center {ENTRIES}")
    lines += [f"property float {name}" for name in NAMES]
    lines.append("end_header")
    return lines


def header(counts, half):
    return ("\n".join(header_lines(counts, half)) + "\n").encode()


def write(path, counts, half, payload):
    assert len(payload) == layout(counts, half)["total"]
    with open(path, "wb") as f:
        f.write(header(counts, half) + np.asarray(payload, np.uint8).tobytes())


def parse(raw):
    """-> (counts, half, payload): reads the header the way the viewer's loader does (the count of each `element vertex` line, f16 on the
    line after it, u8 properties = quantised, the entries of `element cook_center`); asserts the exact size"""
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().split("\n")
    counts, half, entries, quantised = [], False, 0, False
    for k, line in enumerate(lines):
        if line.startswith("element vertex"):
            counts.append(int(line.split()[2]))
            half = half or "f16" in lines[k + 1]
        if line.startswith("property") and line.split()[1] == "u8":
            quantised = True
        if line.startswith("element cook_center"):
            entries = int(line.split()[2])
    assert len(counts) == 4 and quantised and entries == ENTRIES, (counts, quantised, entries)
    payload = np.frombuffer(body, np.uint8)
    assert len(payload) == layout(counts, half)["total"], (len(payload), layout(counts, half)["total"])
    return counts, half, payload


def read(path):
    """-> the decoded model of a file (decode of parse)"""
    counts, half, payload = parse(open(path, "rb").read())
    return decode(payload, counts, half)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def random_model(n, seed=0):
    """values that are multiples of 2^-12 in ranges of a few units (every k(v) is exact), with duplicates"""
    r = np.random.default_rng(seed)
    grid = lambda lo, hi, shape: (r.integers(int(lo * 4096), int(hi * 4096), shape) / 4096.0).astype(f32)
    return {"pos": r.uniform(-4, 4, (n, 3)).astype(f32), "sh0": grid(-2, 2, (n, 3)), "shN": r.uniform(-0.5, 0.5, (n, 45)).astype(f32),
            "opacity": r.uniform(-6, 6, n).astype(f32), "scale": grid(-7, 0, (n, 3)), "rot": r.normal(0, 1, (n, 4)).astype(f32)}


def degree_mix(n, name, seed=0):
    r = np.random.default_rng(seed + 31)
    if name == "all0":
        return np.zeros(n, np.uint8)
    if name == "all3":
        return np.full(n, 3, np.uint8)
    if name == "mixed":                                                      # every block non-empty once n >= 4
        d = r.integers(0, 4, n).astype(np.uint8)
        d[:4] = np.arange(4)[:n]
        return d
    if name == "no2":                                                        # block 2 empty
        return r.choice(np.array([0, 1, 3], np.uint8), n)
    raise KeyError(name)


def degree_case(n, D, C, t=0.01, seed=0):
    """pos, shN, cams for the degree-selection tests: a fifth of the splats each with bands exactly zero from band 1, 2 or 3 upward, a
    fifth with every coefficient at least 10 t / (smallest basis magnitude) — far above t — and a random fifth around t; camera 0 sits
    exactly on splat 0 and is skipped for it."""
    r = np.random.default_rng(1000 * D + 10 * C + seed)
    pos = r.uniform(-2, 2, (n, 3)).astype(f32)
    cams = (r.normal(0, 1, (C, 3)) * 6).astype(f32)
    cams[0] = pos[0]
    shN = np.zeros((n, 15, 3), f32)
    group = np.arange(n) % 5
    big = (r.uniform(2.0, 4.0, (n, 15, 3)) * r.choice([-1.0, 1.0], (n, 15, 3))).astype(f32)
    for g in (0, 1, 2):                                                      # zero from band g + 1 upward, large below
        shN[group == g, :coeffs(g)] = big[group == g, :coeffs(g)]
    shN[group == 3] = big[group == 3]
    shN[group == 4] = r.normal(0, 0.02, (n, 15, 3)).astype(f32)[group == 4]
    shN[:, coeffs(D):] = 0
    return pos, shN.reshape(n, 45), cams


DEGREE_CASES = [(n, D, C) for D in (0, 1, 2, 3) for C in (1, 7, 64) for n in (1, 65, 5000)]
