"""dvs_pack_compressed / dvs_pack_splat32 (csrc/pack.hip) on the GPU against tests/compressed_ply_ref.py, and the plugin's exports end
to end. Compared bit for bit: the Morton order, every chunk row, packed_position, packed_scale, packed_rotation and the three colour
bytes. The alpha byte may differ by one step only where the float64 sigmoid * 255 + 0.5 lies within 1e-3 of an integer (the device
takes the sigmoid in float32), on at most 1 % of the splats. Sizes: 1, one short of / exactly / one past a chunk, 1000, 2049 (past one
2048-key sort partition), 70001 (many partitions and a partial last chunk); the edge inputs of compressed_ply_ref.EDGE_CASES."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import compressed_ply_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")
SIZES = (1, 255, 256, 257, 1000, 2049, 70001)
INVALID = 1                                                  # DVS_ERR_INVALID
GUARD = 16                                                   # 32-bit words kept around every output (64 B: the outputs stay 16-byte aligned)
FIELDS = ("pos", "sh0", "opacity", "scale", "rot")


def _upload(dev, model):
    import torch
    t = [torch.from_numpy(np.ascontiguousarray(model[k], np.float32).reshape(-1)).to(dev) for k in FIELDS]
    assert all(x.data_ptr() % 16 == 0 for x in t)
    return t


def _guarded(dev, words):
    import torch
    buf = torch.full((words + 2 * GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf


def _payload(buf, words):
    h = buf.cpu().numpy().view(np.uint32)
    assert (h[:GUARD] == 0x5A5A5A5A).all() and (h[GUARD + words:] == 0x5A5A5A5A).all(), "a write outside the output"
    return h[GUARD:GUARD + words].copy()


def _pack(dev, model, with_order=True):
    """one dvs_pack_compressed call -> (chunks, verts, order or None); the guard words around every output are checked"""
    import torch
    from divshot_amd._lib import lib
    n = len(np.asarray(model["opacity"]).reshape(-1))
    nch = (n + 255) // 256
    src = _upload(dev, model)
    scratch = torch.empty(lib.dvs_pack_scratch_bytes(n), dtype=torch.uint8, device=dev)
    chunks, verts, order = _guarded(dev, nch * 12), _guarded(dev, n * 4), _guarded(dev, n)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.dvs_pack_compressed(st, n, *[x.data_ptr() for x in src], scratch.data_ptr(), chunks.data_ptr() + 4 * GUARD, verts.data_ptr() + 4 * GUARD,
                                 order.data_ptr() + 4 * GUARD if with_order else None)
    assert rc == 0
    torch.cuda.synchronize()
    o = _payload(order, n)
    if not with_order:
        assert (o == 0x5A5A5A5A).all()
    return _payload(chunks, nch * 12).view(np.float32).reshape(nch, 12), _payload(verts, n * 4).reshape(n, 4), (o if with_order else None)


def _compare(model, got, want=None):
    chunks, verts, order = got
    wc, wv, wo = want if want is not None else R.encode(model)
    n = len(wo)
    if order is not None:
        assert np.array_equal(order, wo), "the Morton order differs"
    assert np.array_equal(chunks.view(np.uint32), wc.view(np.uint32)), "a chunk row differs"
    for col, name in ((0, "packed_position"), (2, "packed_scale"), (1, "packed_rotation")):
        assert np.array_equal(verts[:, col], wv[:, col]), (name, int((verts[:, col] != wv[:, col]).sum()))
    assert np.array_equal(verts[:, 3] >> 8, wv[:, 3] >> 8), "a colour byte differs"
    da = (verts[:, 3] & 255).astype(np.int64) - (wv[:, 3] & 255).astype(np.int64)
    used = da != 0
    slack = R.alpha_slack(np.asarray(model["opacity"]).reshape(-1))[wo.astype(np.int64)]
    print(f"n {n}: alpha bytes off by one {int(used.sum())}, eligible {int(slack.sum())}")
    assert (np.abs(da) <= 1).all() and not used[~slack].any()
    assert used.sum() <= 0.01 * n


@pytest.fixture(scope="module")
def reference():
    """the restatement's encodings, computed once per size"""
    cache = {}

    def get(n):
        if n not in cache:
            m = R.random_model(n, seed=n)
            cache[n] = (m, R.encode(m))
        return cache[n]
    return get


@pytest.mark.parametrize("n", SIZES)
def test_pack_compressed_matches_the_restatement(gpu_device, reference, n):
    model, want = reference(n)
    _compare(model, _pack(gpu_device, model), want)


@pytest.mark.parametrize("name", R.EDGE_CASES)
def test_pack_compressed_edge_inputs(gpu_device, name):
    model = R.edge_model(name)
    got = _pack(gpu_device, model)
    _compare(model, got)
    if name == "one_point":
        assert np.array_equal(got[2], np.arange(len(got[2])))
    if name == "duplicates":                                                 # equal keys stay in index order
        k = R.morton_keys(model["pos"])
        o = got[2].astype(np.int64)
        assert all((np.diff(o[k[o] == v]) > 0).all() for v in np.unique(k))


def test_null_order_and_repeatability(gpu_device, reference):
    model, want = reference(2049)
    a, b, c = _pack(gpu_device, model), _pack(gpu_device, model), _pack(gpu_device, model, with_order=False)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()                                    # two calls, identical bytes
    assert c[2] is None and c[0].tobytes() == a[0].tobytes() and c[1].tobytes() == a[1].tobytes()
    _compare(model, c, want)


def test_morton_order_users_do_not_share_state(gpu_device):
    """dvs_pack_compressed and dvs_knn_mean_dist2 both sort through dvs_launch_morton_order, each in its own scratch: run one after the
    other (and the packer once more after the search) on the same 2049 positions, a third of them repeated — past one 2048-key sort
    partition, with ties —, each equals its restatement whatever the other left behind."""
    import torch
    import knn_ref as K
    from divshot_amd._lib import lib
    n = 2049
    model = R.random_model(n, seed=77)
    rng = np.random.default_rng(78)
    pos = np.array(model["pos"], np.float32).reshape(n, 3)
    pos[rng.integers(0, n, n // 3)] = pos[0]
    model["pos"] = pos
    want = R.encode(model)
    _compare(model, _pack(gpu_device, model), want)
    d_pos = torch.from_numpy(pos.reshape(-1).copy()).to(gpu_device)
    scratch = torch.empty(lib.dvs_knn_scratch_bytes(n), dtype=torch.uint8, device=gpu_device)
    dist2 = _guarded(gpu_device, n)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.dvs_knn_mean_dist2(st, n, d_pos.data_ptr(), scratch.data_ptr(), dist2.data_ptr() + 4 * GUARD) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_payload(dist2, n), K.mean_dist2(pos).view(np.uint32)), "dist2 differs from the all-pairs restatement"
    _compare(model, _pack(gpu_device, model), want)


def test_invalid_arguments(gpu_device):
    import torch
    from divshot_amd._lib import lib
    n = 300
    keep = _upload(gpu_device, R.random_model(n, seed=1))
    src = [x.data_ptr() for x in keep]
    scratch = torch.empty(lib.dvs_pack_scratch_bytes(n), dtype=torch.uint8, device=gpu_device)
    out = torch.zeros(n * 16 + 64, dtype=torch.int32, device=gpu_device)
    chunks, verts, order = out.data_ptr(), out.data_ptr() + 4096, out.data_ptr() + 4096 + n * 16
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = src + [scratch.data_ptr(), chunks, verts, order]
    assert lib.dvs_pack_compressed(st, n, *good) == 0
    assert lib.dvs_pack_scratch_bytes(0) == 0 and lib.dvs_pack_scratch_bytes(-5) == 0 and lib.dvs_pack_scratch_bytes(n) % 16 == 0
    for bad_n in (0, -1):
        assert lib.dvs_pack_compressed(st, bad_n, *good) == INVALID
        assert lib.dvs_pack_splat32(st, bad_n, *src, out.data_ptr()) == INVALID
    for i in range(len(good)):
        args = list(good)
        args[i] = good[i] + 4                                                # off a 16-byte boundary
        assert lib.dvs_pack_compressed(st, n, *args) == INVALID, i
        if i < len(good) - 1:                                                # every pointer but `order` is required
            args[i] = None
            assert lib.dvs_pack_compressed(st, n, *args) == INVALID, i
    for i in range(6):
        args = src + [out.data_ptr()]
        args[i] = args[i] + 4
        assert lib.dvs_pack_splat32(st, n, *args) == INVALID, i
        args[i] = None
        assert lib.dvs_pack_splat32(st, n, *args) == INVALID, i
    torch.cuda.synchronize()
    del keep


SPLAT_CASES = [("random", 1), ("random", 257), ("random", 70001), ("zero_quat", 777), ("negative_largest", 777), ("equal_magnitude", 777),
               ("sh0_saturated", 777)]


@pytest.mark.parametrize("name,n", SPLAT_CASES)
def test_pack_splat32_matches_the_restatement(gpu_device, name, n):
    """Bytes 0-11 and 28-31 bit for bit; the colour bytes 24-27 with the one-step allowance where the float64 value before truncation lies
    within 1e-3 of an integer, on at most 1 % of the splats; exp(scale) within 4 ulp of the float64 exp (the device's exp is < 2 ulp).
    (Logits of +-20 are left to the compressed format's cases: sigmoid(20) * 255 = 254.9999995 truncates to 254 in float64 and to 255
    from any float32 sigmoid, the reference's own included — every such splat would need the allowance.)"""
    import torch
    from divshot_amd._lib import lib
    model = R.random_model(n, seed=n) if name == "random" else R.edge_model(name, n)
    src = _upload(gpu_device, model)
    out = _guarded(gpu_device, n * 8)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.dvs_pack_splat32(st, n, *[x.data_ptr() for x in src], out.data_ptr() + 4 * GUARD) == 0
    torch.cuda.synchronize()
    got = _payload(out, n * 8).view(np.uint8).reshape(n, 32)
    want = R.encode_splat32(model)
    assert np.array_equal(got[:, 0:12], want[:, 0:12]) and np.array_equal(got[:, 28:32], want[:, 28:32])
    d = got[:, 24:28].astype(np.int64) - want[:, 24:28].astype(np.int64)
    used = d != 0
    print(f"n {n}: colour bytes off by one {int(used.sum())}, eligible {int(R.splat32_slack(model).sum())}")
    assert (np.abs(d) <= 1).all() and not used[~R.splat32_slack(model)].any()
    assert used.any(axis=1).sum() <= 0.01 * n
    e_got = np.ascontiguousarray(got[:, 12:24]).view(np.float32).reshape(n, 3)
    e_ref = np.exp(np.asarray(model["scale"], np.float64).reshape(n, 3))
    assert (np.abs(e_got.astype(np.float64) - e_ref) <= 4 * np.spacing(e_ref.astype(np.float32))).all()


# ---- the plugin end to end -------------------------------------------------------------------------------------------------------
SCENE = ["--inputPath", "synthetic:N=2000,W=64,H=64,cams=4,sh=1,seed=1", "--maxIteration", "30"]


def _run(args):
    p = subprocess.run([DRIVER] + SCENE + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p


def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int(re.search(rb"element vertex (\d+)", head).group(1))
    row = np.frombuffer(body, np.float32).reshape(n, 59)
    return {"pos": row[:, 0:3], "sh0": row[:, 3:6], "opacity": row[:, 51], "scale": row[:, 52:55], "rot": row[:, 55:59]}


def test_plugin_writes_the_selected_formats(gpu_device, tmp_path):
    """--exportFormat compressed,splat: the three files of iteration 30 exist with exact sizes; the decoded compressed file, un-permuted
    by the Morton order of the PLY's positions, lies within the format's bounds of the full PLY; the .splat records equal the
    restatement's on the PLY. A modelPath ending in .compressed.ply and no flag writes the compressed file (the editor's route); a run
    with neither writes the PLY alone and logs no export line."""
    out = str(tmp_path / "a" / "iteration")
    p = _run(["--outputPath", out, "--exportFormat", "compressed,splat"])
    model = _read_ply(out + "_30.ply")
    n = len(model["opacity"])
    assert n == 2000
    chunks, verts = R.read_compressed_ply(out + "_30.compressed.ply")       # (asserts the exact header and size)
    assert len(verts) == n and os.path.getsize(out + "_30.splat") == 32 * n
    assert os.path.getsize(out + "_30.compressed.ply") == len(R.header(n)) + 48 * ((n + 255) // 256) + 16 * n
    R.assert_within_format_bounds(model, chunks, verts, R.morton_order(model["pos"]))
    _compare(model, (chunks, verts, None))
    rec = np.fromfile(out + "_30.splat", np.uint8).reshape(n, 32)
    want = R.encode_splat32(model)
    assert np.array_equal(rec[:, 0:12], want[:, 0:12]) and np.array_equal(rec[:, 28:32], want[:, 28:32])
    d = rec[:, 24:28].astype(np.int64) - want[:, 24:28]
    assert (np.abs(d) <= 1).all() and not (d != 0)[~R.splat32_slack(model)].any()
    logs = [l for l in p.stderr.splitlines() if "export @30:" in l]              # the full PLY's own line first: the comparison
    assert len(logs) == 3 and "export @30: ply 2000 splats" in logs[0] and "export @30: splat 2000 splats" in logs[2]
    assert re.search(r"export @30: compressed\.ply 2000 splats, \d+ bytes, [\d.]+ ms", logs[1])
    assert "config: exportFormats 3" in p.stderr

    out_b = str(tmp_path / "b" / "scene.compressed.ply")
    pb = _run(["--outputPath", out_b])
    assert os.path.exists(out_b + "_30.ply") and os.path.exists(out_b + "_30.compressed.ply") and not os.path.exists(out_b + "_30.splat")
    assert "turned on by the suffix of modelPath" in pb.stderr
    cb, vb = R.read_compressed_ply(out_b + "_30.compressed.ply")
    _compare(_read_ply(out_b + "_30.ply"), (cb, vb, None))

    out_c = str(tmp_path / "c" / "iteration")
    pc = _run(["--outputPath", out_c])
    assert sorted(os.listdir(str(tmp_path / "c"))) == ["iteration_30.ply"]
    assert "export" not in pc.stderr and "export" not in pc.stdout
