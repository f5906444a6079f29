"""dvs_pack_spz / dvs_unpack_spz (csrc/pack.hip) on the GPU against tests/spz_ref.py, and the plugin's .spz export end to end.
Compared bit for bit: every packed section but the alpha byte, which may differ by one step only where the float64 sigmoid * 255 lies
within 1e-3 of k + 1/2 (the device takes the sigmoid in float32), on at most 1 % of the splats; every decoded array but the opacity logit
and the reconstructed quaternion component, both within 2 ulp (log and sqrt of another library). Sizes: one lane, a partial tile, an exact
tile, a tile plus a tail, several workgroups plus a tail; both shN layouts; degrees 0..3."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import numpy as np
import pytest
import spz_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")
SIZES = (1, 63, 64, 65, 1000, 2049)
ROWS, TILED = 0, 1
INVALID = 1                                                  # DVS_ERR_INVALID
GUARD = 64                                                   # bytes kept around every device buffer (the payload stays 16-byte aligned)
FILL = 0x5A
f32 = np.float32


def _tiled(shN, pad=0.0):
    """[n][45] -> DVS_SHN_TILED: element e of splat i at (((i >> 6) * 12 + e / 4) * 64 + (i & 63)) * 4 + e % 4; whole tiles."""
    shN = np.asarray(shN, f32).reshape(-1, 45)
    n = len(shN)
    tiles = (n + 63) // 64
    full = np.full((tiles * 64, 48), pad, f32)
    full[:n, :45] = shN
    return np.ascontiguousarray(full.reshape(tiles, 64, 12, 4).transpose(0, 2, 1, 3)).reshape(-1)


def _guarded(dev, nbytes):
    import torch
    buf = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf


def _payload(buf, nbytes):
    h = buf.cpu().numpy()
    assert (h[:GUARD] == FILL).all() and (h[GUARD + nbytes:] == FILL).all(), "a write outside the buffer"
    return h[GUARD:GUARD + nbytes].copy()


def _upload(dev, model, layout):
    import torch
    arrs = {k: np.ascontiguousarray(model[k], f32).reshape(-1) for k in S.FIELDS}
    arrs["shN"] = _tiled(model["shN"], pad=9.0) if layout == TILED else arrs["shN"]       # (the pads are never packed)
    t = {k: torch.from_numpy(v).to(dev) for k, v in arrs.items()}
    assert all(x.data_ptr() % 16 == 0 for x in t.values())
    return t


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _pack(dev, model, degree, layout):
    """one dvs_pack_spz call -> dict of sections; the guard bytes around the buffer and the gaps between its sections are checked"""
    import torch
    from divshot_amd._lib import lib, SpzLayout
    n = len(np.asarray(model["opacity"]).reshape(-1))
    L = SpzLayout()
    assert lib.dvs_spz_layout_for(n, degree, C.byref(L)) == 0
    off, size, total = S.layout(n, degree)
    assert (list(L.off), list(L.bytes), L.total) == (off, size, total)
    src = _upload(dev, model, layout)
    out = _guarded(dev, total)
    rc = lib.dvs_pack_spz(_stream(), n, degree, src["pos"].data_ptr(), src["sh0"].data_ptr(), src["shN"].data_ptr(), layout,
                          src["opacity"].data_ptr(), src["scale"].data_ptr(), src["rot"].data_ptr(), out.data_ptr() + GUARD)
    assert rc == 0
    torch.cuda.synchronize()
    raw = _payload(out, total)
    ends = off[1:] + [total]
    for k in range(6):
        assert (raw[off[k] + size[k]:ends[k]] == FILL).all(), f"a write past section {S.SECTIONS[k]}"
    return {name: raw[o:o + b] for name, o, b in zip(S.SECTIONS, off, size)}


def _compare_packed(model, got, want):
    n = len(want["alphas"])
    for name in S.SECTIONS:
        assert got[name].shape == want[name].shape, name
        if name != "alphas":
            assert np.array_equal(got[name], want[name]), (name, int((got[name] != want[name]).sum()))
    d = got["alphas"].astype(np.int64) - want["alphas"].astype(np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        slack = S.alpha_slack(np.asarray(model["opacity"]).reshape(-1))
    print(f"n {n}: alpha bytes off by one {int((d != 0).sum())}, eligible {int(slack.sum())}")
    assert (np.abs(d) <= 1).all() and not (d != 0)[~slack].any()
    assert (d != 0).sum() <= 0.01 * n


def _unpack(dev, sec, n, degree, layout, with_shn=True):
    """one dvs_unpack_spz call on the sections laid out as the device buffer -> dict of arrays (shN as the device holds it)"""
    import torch
    from divshot_amd._lib import lib
    off, size, total = S.layout(n, degree)
    raw = np.full(total, 0xEE, np.uint8)
    for name, o, b in zip(S.SECTIONS, off, size):
        raw[o:o + b] = sec[name]
    packed = torch.from_numpy(raw).to(dev)
    shn_floats = (n + 63) // 64 * 64 * 48 if layout == TILED else n * 45
    floats = {"pos": 3 * n, "sh0": 3 * n, "shN": shn_floats, "opacity": n, "scale": 3 * n, "rot": 4 * n}
    out = {k: _guarded(dev, 4 * v) for k, v in floats.items()}
    ptr = {k: out[k].data_ptr() + GUARD for k in out}
    rc = lib.dvs_unpack_spz(_stream(), n, degree, packed.data_ptr(), ptr["pos"], ptr["sh0"], ptr["shN"] if with_shn else None, layout,
                            ptr["opacity"], ptr["scale"], ptr["rot"])
    assert rc == 0
    torch.cuda.synchronize()
    return {k: _payload(out[k], 4 * floats[k]).view(f32) for k in out}


def _ulp_close(got, want, ulps):
    fin = np.isfinite(want)
    return np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin]) and \
        (np.abs(got[fin].astype(np.float64) - want[fin]) <= ulps * np.spacing(np.abs(want[fin]))).all()


def _compare_unpacked(got, want, n, layout):
    for k in ("pos", "sh0", "scale"):
        assert np.array_equal(got[k].view(np.uint32), want[k].reshape(-1).view(np.uint32)), k
    shn = _tiled(want["shN"]) if layout == TILED else want["shN"].reshape(-1)             # pads, lanes past n, absent bands: exactly 0
    assert np.array_equal(got["shN"].view(np.uint32), shn.view(np.uint32)), "shN"
    assert _ulp_close(got["opacity"], want["opacity"], 2)
    rebuilt = np.zeros((n, 4), bool)
    rebuilt[np.arange(n), (want["largest"] + 1) % 4] = True
    rot = got["rot"].reshape(n, 4)
    assert np.array_equal(rot[~rebuilt].view(np.uint32), want["rot"][~rebuilt].view(np.uint32))
    assert _ulp_close(rot[rebuilt], want["rot"][rebuilt], 2)


@pytest.fixture(scope="module")
def reference():
    """the restatement's packings and decodings, computed once per (size, degree)"""
    cache = {}

    def get(n, degree):
        if (n, degree) not in cache:
            m = S.random_model(n, seed=n)
            packed = S.pack(m, degree)
            cache[(n, degree)] = (m, packed, S.unpack(packed, degree))
        return cache[(n, degree)]
    return get


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("layout", [ROWS, TILED])
@pytest.mark.parametrize("n", SIZES)
def test_pack_spz_matches_the_restatement(gpu_device, reference, n, layout, degree):
    model, want, _ = reference(n, degree)
    _compare_packed(model, _pack(gpu_device, model, degree, layout), want)


@pytest.mark.parametrize("layout", [ROWS, TILED])
@pytest.mark.parametrize("name", S.EDGE_CASES)
def test_pack_spz_edge_inputs(gpu_device, name, layout):
    """NaN / +inf / -inf in each array, zero and overflowing quaternions, |pos| >= 2048, logits +-30, all-equal quaternion components:
    the header's rule for every case the reference leaves undefined, twice with identical bytes; then the decode of that payload."""
    model = S.edge_model(name)
    n = len(model["opacity"])
    with np.errstate(over="ignore", invalid="ignore"):
        want = S.pack(model, 3)
    a, b = _pack(gpu_device, model, 3, layout), _pack(gpu_device, model, 3, layout)
    for k in S.SECTIONS:
        assert a[k].tobytes() == b[k].tobytes(), k                           # two calls, identical bytes
    _compare_packed(model, a, want)
    _compare_unpacked(_unpack(gpu_device, a, n, 3, layout), S.unpack(a, 3), n, layout)


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("layout", [ROWS, TILED])
@pytest.mark.parametrize("n", SIZES)
def test_unpack_spz_matches_the_restatement(gpu_device, reference, n, layout, degree):
    _, packed, want = reference(n, degree)
    _compare_unpacked(_unpack(gpu_device, packed, n, degree, layout), want, n, layout)


def test_degree_0_takes_a_null_shn(gpu_device, reference):
    import torch
    from divshot_amd._lib import lib
    model, want, dec = reference(65, 0)
    src = _upload(gpu_device, model, ROWS)
    out = _guarded(gpu_device, S.layout(65, 0)[2])
    assert lib.dvs_pack_spz(_stream(), 65, 0, src["pos"].data_ptr(), src["sh0"].data_ptr(), None, ROWS, src["opacity"].data_ptr(),
                            src["scale"].data_ptr(), src["rot"].data_ptr(), out.data_ptr() + GUARD) == 0
    torch.cuda.synchronize()
    raw = _payload(out, S.layout(65, 0)[2])
    off, size, _ = S.layout(65, 0)
    assert all(np.array_equal(raw[o:o + b], want[k]) for k, o, b in zip(S.SECTIONS, off, size) if k != "alphas")
    got = _unpack(gpu_device, want, 65, 0, ROWS, with_shn=False)
    assert (got["shN"].view(np.uint8) == FILL).all()                          # not touched
    assert np.array_equal(got["pos"].view(np.uint32), dec["pos"].reshape(-1).view(np.uint32))


def test_invalid_arguments(gpu_device):
    import torch
    from divshot_amd._lib import lib, SpzLayout
    n = 100
    L = SpzLayout()
    for bad in ((0, 3), (-1, 3), (n, -1), (n, 4)):
        assert lib.dvs_spz_layout_for(bad[0], bad[1], C.byref(L)) == INVALID
    assert lib.dvs_spz_layout_for(n, 3, None) == INVALID
    src = _upload(gpu_device, S.random_model(n, seed=1), ROWS)
    out = _guarded(gpu_device, S.layout(n, 3)[2])
    dst = {k: torch.zeros(src[k].numel() + 16, dtype=torch.float32, device=gpu_device) for k in S.FIELDS}
    st = _stream()
    p = lambda t: t.data_ptr()
    pack_args = [p(src["pos"]), p(src["sh0"]), p(src["shN"]), ROWS, p(src["opacity"]), p(src["scale"]), p(src["rot"]), out.data_ptr() + GUARD]
    unpack_args = [out.data_ptr() + GUARD, p(dst["pos"]), p(dst["sh0"]), p(dst["shN"]), ROWS, p(dst["opacity"]), p(dst["scale"]), p(dst["rot"])]
    assert lib.dvs_pack_spz(st, n, 3, *pack_args) == 0 and lib.dvs_unpack_spz(st, n, 3, *unpack_args) == 0
    torch.cuda.synchronize()
    before = out.cpu().numpy().copy()
    for fn, good, layout_at in ((lib.dvs_pack_spz, pack_args, 3), (lib.dvs_unpack_spz, unpack_args, 4)):
        for bad_n, bad_deg in ((0, 3), (-5, 3), (n, -1), (n, 4)):
            assert fn(st, bad_n, bad_deg, *good) == INVALID
        for i in range(len(good)):
            args = list(good)
            if i == layout_at:
                for bad_layout in (-1, 2):
                    args[i] = bad_layout
                    assert fn(st, n, 3, *args) == INVALID
                continue
            args[i] = good[i] + 4                                            # off a 16-byte boundary
            assert fn(st, n, 3, *args) == INVALID, i
            args[i] = None
            assert fn(st, n, 3, *args) == INVALID, i                         # (shN too: NULL only at degree 0)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), before)                         # nothing was launched


# ---- the plugin end to end -------------------------------------------------------------------------------------------------------
SCENE = ["--inputPath", "synthetic:N=2000,W=64,H=64,cams=8,sh=2,seed=1", "--maxIteration", "30", "--eval"]
# The decoded model's held-out PSNR drop on this run, full model minus decoded .spz model, measured once on an MI355X (full model
# 29.659310 dB, decoded 29.624333 dB; SSIM 0.944459 -> 0.943987): see test_fidelity_of_the_decoded_model.
RECORDED_DROP_DB = 0.034977


def _run(args, env=None):
    e = dict(os.environ)
    e.pop("DVS_EXPORT_FORMATS", None)
    e.update(env or {})
    p = subprocess.run([DRIVER] + SCENE + args, capture_output=True, text=True, timeout=300, env=e)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p


def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int(re.search(rb"element vertex (\d+)", head).group(1))
    row = np.frombuffer(body, f32).reshape(n, 59)
    shN = np.ascontiguousarray(row[:, 6:51].reshape(n, 3, 15).transpose(0, 2, 1)).reshape(n, 45)       # f_rest is channel-major on disk
    return {"pos": row[:, 0:3], "sh0": row[:, 3:6], "shN": shN, "opacity": row[:, 51], "scale": row[:, 52:55], "rot": row[:, 55:59]}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The same 30 iterations with and without --exportSpz, and a third run without the switch that resumes from the first one's model
    at iteration 30 and saves at once. Two trainings of this build are not comparable bit for bit (the composite backward's fp32 atomics
    add in an order that differs from run to run), so the run whose evaluation must EQUAL the first one's is the one
    that scores the very same parameters."""
    base = tmp_path_factory.mktemp("spz")
    on, off, same = (str(base / t / "iteration") for t in ("on", "off", "same"))
    p_on, p_off = _run(["--outputPath", on, "--exportSpz"]), _run(["--outputPath", off])
    os.makedirs(os.path.dirname(same))
    shutil.copy(on + "_30.ply", same + "_30.ply")
    p_same = _run(["--outputPath", same, "--load_itr", "30"])
    assert "(resumed)" in p_same.stderr, p_same.stderr[-3000:]
    return on, p_on, off, p_off, same


def test_plugin_writes_the_spz_file(gpu_device, runs):
    """<out>_30.spz holds the restatement's packing of <out>_30.ply at the model's degree; the eval JSON gains exports.spz and keeps its
    views / mean blocks (equal to those of a run without the switch on the same parameters); the same run without the switch writes
    no .spz, no exports key and no export line."""
    on, p, off, q, same = runs
    model = _read_ply(on + "_30.ply")
    n, degree, aa, sec = S.read_spz(on + "_30.spz")                          # (asserts the header and the exact size)
    assert (n, degree, aa) == (2000, 2, False) and len(model["opacity"]) == n
    _compare_packed(model, sec, S.pack(model, 2))
    m = re.search(r"export @30: spz 2000 splats, (\d+) bytes, [\d.]+ ms", p.stderr)
    assert m and int(m.group(1)) == os.path.getsize(on + "_30.spz"), p.stderr[-3000:]
    assert "config: exportFormats 4" in p.stderr and not [l for l in p.stderr.splitlines() if "IGNORED" in l and "spz" in l]
    J, K = json.load(open(on + "_30_eval.json")), json.load(open(off + "_30_eval.json"))
    assert set(J["exports"]) == {"spz"} and set(J["exports"]["spz"]) == {"psnr", "ssim", "l1", "mse"}
    assert all(np.isfinite(v) for v in J["exports"]["spz"].values())
    assert "exports" not in K and set(J) - {"exports"} == set(K)
    K2 = json.load(open(same + "_30_eval.json"))                             # the same parameters scored by a run without the switch
    assert open(same + "_30.ply", "rb").read() == open(on + "_30.ply", "rb").read()
    assert J["views"] == K2["views"] and J["mean"] == K2["mean"] and {k: v for k, v in J.items() if k != "exports"} == K2
    assert sorted(os.listdir(os.path.dirname(off))) == ["iteration_30.ply", "iteration_30_eval.json"]
    assert "export" not in q.stderr and "export" not in q.stdout


def test_model_path_suffix_turns_the_export_on(gpu_device, tmp_path):
    out = str(tmp_path / "scene.spz")
    p = _run(["--outputPath", out])
    assert os.path.exists(out + "_30.ply") and os.path.exists(out + "_30.spz")
    assert "turned on by the suffix of modelPath" in p.stderr and "config: exportFormats 4" in p.stderr
    assert not [l for l in p.stderr.splitlines() if "IGNORED" in l and ".spz" in l]
    n, degree, _, sec = S.read_spz(out + "_30.spz")
    _compare_packed(_read_ply(out + "_30.ply"), sec, S.pack(_read_ply(out + "_30.ply"), degree))


def test_fidelity_of_the_decoded_model(gpu_device, runs):
    """What the compact file costs: the held-out PSNR of the model decoded from the .spz payload against the full model's of the same
    run. Quantisation cannot help beyond noise (<= full + 0.01 dB); the drop stays within twice the one measured once on an MI355X on
    this run (RECORDED_DROP_DB = 0.034977 dB: 29.659310 dB -> 29.624333 dB on camera 0, the one held-out view of the 8; the factor 2
    covers the run-to-run variation of a 30-iteration model); and the two scores are not bit-equal
    (the decoded set was really rendered)."""
    on, p = runs[0], runs[1]
    J = json.load(open(on + "_30_eval.json"))
    full, spz = J["mean"]["psnr"], J["exports"]["spz"]["psnr"]
    m = re.search(r"export @30: spz decoded model: PSNR (\S+) dB \(full model (\S+) dB\), SSIM (\S+), L1 (\S+)", p.stderr)
    assert m, p.stderr[-3000:]
    print(f"held-out PSNR: full model {full:.6f} dB, decoded .spz model {spz:.6f} dB, drop {full - spz:.6f} dB; "
          f"SSIM {J['mean']['ssim']:.6f} -> {J['exports']['spz']['ssim']:.6f}")
    assert float(m.group(1)) == spz and float(m.group(2)) == full
    assert spz != full
    assert spz <= full + 0.01
    assert full - spz <= 2 * RECORDED_DROP_DB
