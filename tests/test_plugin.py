"""B1 — the `gstrain` plugin boundary: exported symbols, PLY wire format (KAT-5), and — on the GPU —
the full host call sequence of diverseshot-cli driving a short synthetic training run."""
import ctypes as C
import os
import re
import struct
import subprocess
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "divshot_amd", "lib")
PLUGIN = os.path.join(LIB, "libgstrain.so")
DRIVER = os.path.join(LIB, "gaussian_train")


@pytest.fixture(scope="module")
def plugin():
    if not os.path.exists(PLUGIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "divshot_amd", "gstrain")])
    return C.CDLL(PLUGIN)


def test_plugin_exports_the_host_symbols(plugin):
    # gs_train.cpp:24,105-109,144-150,178 + plugin.cpp:89-111
    for name in ("gstrain_init", "create_splat", "load_train_data", "train_step", "get_cur_step", "save_splat_model",
                 "export_mesh", "delete_splat", "gstrain_destroy", "get_description", "create_instance"):
        assert hasattr(plugin, name), name
    plugin.get_description.restype = C.c_char_p
    assert b"gstrain" in plugin.get_description()


def test_kat5_ply_wire_format(plugin, tmp_path):
    """external/tinygsplat/tiny_gsplat.cpp:194-216 property order, 59 floats = 236 B per vertex, f_rest channel-major on disk
    ([c*15+j], tiny_gsplat.cpp:231-236) vs coefficient-major in memory ([j*3+c], gaussian_model.cpp:163-167)."""
    n = 257
    rng = np.random.default_rng(5)
    A = {"pos": rng.normal(size=(n, 3)), "sh0": rng.normal(size=(n, 3)), "shN": rng.normal(size=(n, 15, 3)),
         "opacity": rng.normal(size=(n,)), "scale": rng.normal(size=(n, 3)), "rot": rng.normal(size=(n, 4))}
    A = {k: np.ascontiguousarray(v, np.float32) for k, v in A.items()}
    path = str(tmp_path / "m.ply").encode()
    order = ("pos", "sh0", "shN", "opacity", "scale", "rot")
    plugin.gstrain_write_ply.argtypes = [C.c_char_p, C.c_uint64] + [C.c_void_p] * 6 + [C.c_int]
    assert plugin.gstrain_write_ply(path, n, *[A[k].ctypes.data for k in order], 1) == 0
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().strip().split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    assert "comment splatx.anti_aliasing=1" in lines and f"element vertex {n}" in lines
    props = [l.split()[-1] for l in lines if l.startswith("property float")]
    want = ["x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(45)] + ["opacity", "scale_0", "scale_1", "scale_2",
                                                                                                 "rot_0", "rot_1", "rot_2", "rot_3"]
    assert props == want
    assert len(body) == n * 236
    row = np.frombuffer(body, np.float32).reshape(n, 59)
    assert np.array_equal(row[:, 0:3], A["pos"]) and np.array_equal(row[:, 3:6], A["sh0"])
    assert np.array_equal(row[:, 6:51].reshape(n, 3, 15), A["shN"].transpose(0, 2, 1))       # f_rest[c*15+j] = shN[j][c]
    assert np.array_equal(row[:, 51], A["opacity"]) and np.array_equal(row[:, 52:55], A["scale"]) and np.array_equal(row[:, 55:59], A["rot"])
    B = {k: np.zeros_like(v) for k, v in A.items()}
    plugin.gstrain_read_ply.restype = C.c_int64
    plugin.gstrain_read_ply.argtypes = [C.c_char_p] + [C.c_void_p] * 6 + [C.c_uint64]
    assert plugin.gstrain_read_ply(path, *[B[k].ctypes.data for k in order], n) == n
    for k in order:
        assert np.array_equal(A[k], B[k]), k


HOST_SRC = os.path.join(ROOT, "tests", "hosts", "editor_like.cpp")


def build_editor_like(dst):
    """The editor-like host links libgstrain DIRECTLY (no dlsym): the class, its getters and the two free probes must be exported."""
    exe = os.path.join(str(dst), "editor_like")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), HOST_SRC, "-o", exe, "-L", LIB, "-lgstrain",
                           "-Wl,-rpath," + LIB, "-Wl,-rpath-link," + LIB])
    return exe


def test_cpp_trainer_surface_is_exported(plugin, tmp_path):
    """SURVEY §8(f) rank 4 / VERDICT r05 item 1: the reference's second host constructs GaussianTrainerScene itself (editor.cpp:2023) and
    calls its methods (editor.cpp:1459-1473, inspector_panel.cpp:765-1000) — every public member function the header declares, the two
    free probes (editor.cpp:1534,1539) and the C symbols are dynamic symbols of libgstrain.so; the implementation struct and the PLY
    code are not. The exported set is pinned: additions are deliberate."""
    out = subprocess.check_output(["nm", "-DC", "--defined-only", PLUGIN]).decode()
    syms = [l.split(None, 2)[2] for l in out.splitlines() if len(l.split(None, 2)) == 3 and l.split(None, 2)[1] in "TWV"]
    methods = sorted({re.match(r"GaussianTrainerScene::(~?\w+)", s_).group(1) for s_ in syms if s_.startswith("GaussianTrainerScene::")})
    hdr = open(os.path.join(ROOT, "include", "gaussian_trainer_scene.hpp")).read()
    body = re.sub(r"//[^\n]*", "", hdr[hdr.index("class GSTRAIN_API GaussianTrainerScene"):hdr.index("private:")])
    declared = sorted(set(re.findall(r"(~?\b[A-Za-z_]\w*)\s*\([^;{]*\)\s*(?:const)?\s*;", body)) - {"operator"})
    assert "getGaussianSHNCpu" in declared and "GaussianTrainerScene" in declared and "~GaussianTrainerScene" in declared and len(declared) >= 40
    assert methods == declared, (sorted(set(declared) - set(methods)), sorted(set(methods) - set(declared)))
    free = sorted(s_.split("(")[0] for s_ in syms if not s_.startswith("GaussianTrainerScene::") and "Impl" not in s_
                  and not s_.startswith(("typeinfo", "vtable", "std::", "void std::", "guard variable")))
    assert free == sorted(["gstrain_init", "create_splat", "load_train_data", "train_step", "get_cur_step", "save_splat_model", "export_mesh",
                           "delete_splat", "gstrain_destroy", "get_description", "create_instance", "gstrain_write_ply", "gstrain_read_ply",
                           "is_device_support_gstrain", "is_driver_support"]), free
    assert not any("::Impl::" in s_ or "gsply" in s_ for s_ in syms)
    # and a host that links the class directly builds; without a device it refuses loudly (no CPU path)
    exe = build_editor_like(tmp_path)
    import torch
    if not torch.cuda.is_available():
        p = subprocess.run([exe, "synthetic:N=100,W=64,H=64,cams=2,sh=1,seed=1", str(tmp_path / "m"), "1", "1", str(tmp_path / "d")], capture_output=True, text=True)
        assert p.returncode == 3 and "no supported device" in p.stderr


def read_editor_dump(path):
    raw = open(path, "rb").read()
    n = int(np.frombuffer(raw[:8], np.int64)[0])
    a = np.frombuffer(raw[8:], np.float32)
    assert a.size == n * 59, (a.size, n)
    out, o = {}, 0
    for k, w in (("pos", 3), ("sh0", 3), ("shN", 45), ("opacity", 1), ("scale", 3), ("rot", 4)):       # the dump's order, not the PLY's
        out[k] = a[o:o + n * w].reshape(n, w); o += n * w
    return n, out


@pytest.mark.gpu
def test_editor_like_host_pulls_the_model_through_the_getters(plugin, tmp_path):
    """The trainer -> viewer hand-off of editor.cpp:1459-1473 -> GaussianModel::update_from_cpu (gaussian_model.cpp:43-68): a host linked
    against libgstrain constructs the class with (cfg, -1), loads, trains across an ADC refinement (so that N changes), pulls the six arrays
    with the editor's byte counts (12 / 16 / 12 / 4 / 12 / 180 B per splat) and saves. What the viewer-side container received equals the
    PLY of the same iteration BIT FOR BIT — in particular shs_n[j*3+c] after the un-tiling of the training layout (DVS_SHN_TILED)."""
    exe = build_editor_like(tmp_path)
    model, dump = str(tmp_path / "m" / "iteration"), str(tmp_path / "dump")
    p = subprocess.run([exe, "synthetic:N=6000,W=192,H=128,cams=6,sh=3,seed=11", model, "7", "8", dump], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"splats (\d+) -> (\d+) -> (\d+), iterations (\d+), loss ([0-9.eE+-]+), status (\d+)", p.stdout)
    assert m, p.stdout
    n0, n1, n2, its = (int(m.group(k)) for k in range(1, 5))
    assert n0 == n1 == 6000 and n2 != n1 and its == 15 and float(m.group(5)) > 0, p.stdout      # the refinement at iteration 10 changed N
    plugin.gstrain_read_ply.restype = C.c_int64
    plugin.gstrain_read_ply.argtypes = [C.c_char_p] + [C.c_void_p] * 6 + [C.c_uint64]
    order = ("pos", "sh0", "shN", "opacity", "scale", "rot")
    for tag, it, n_want in (("a", 7, n1), ("b", 15, n2)):
        n, got = read_editor_dump(f"{dump}_{tag}.bin")
        assert n == n_want
        ply = {k: np.zeros_like(got[k]) for k in order}
        assert plugin.gstrain_read_ply(f"{model}_{it}.ply".encode(), *[ply[k].ctypes.data for k in order], n) == n
        for k in order:
            assert np.array_equal(got[k].view(np.uint32), ply[k].view(np.uint32)), (tag, k)
        assert np.abs(got["shN"]).max() > 0 and np.isfinite(got["shN"]).all()
        # the raw file agrees too: f_rest[c*15+j] on disk = shs_n[j*3+c] in the viewer (tiny_gsplat.cpp:231-236, gaussian_model.cpp:163-167)
        raw = open(f"{model}_{it}.ply", "rb").read().split(b"end_header\n", 1)[1]
        row = np.frombuffer(raw, np.float32).reshape(n, 59)
        assert np.array_equal(row[:, 6:51].reshape(n, 3, 15), got["shN"].reshape(n, 15, 3).transpose(0, 2, 1))
    a, b = read_editor_dump(dump + "_a.bin")[1], read_editor_dump(dump + "_b.bin")[1]
    assert not np.array_equal(a["pos"][:100], b["pos"][:100]) or n2 != n1                        # the getters are not serving a stale copy


@pytest.mark.gpu
def test_cli_trains_synthetic_scene(tmp_path):
    """The host sequence init -> create -> load -> {get_cur_step, train_step}* -> save -> delete -> destroy, end to end."""
    out = str(tmp_path / "model" / "iteration")
    cmd = [DRIVER, "--inputPath", "synthetic:N=20000,W=256,H=256,cams=4,sh=1,seed=3", "--maxIteration", "400", "--outputPath", out]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    losses = [float(m.group(2)) for m in re.finditer(r"Iteraions (\d+), loss : ([0-9.eE+-]+)", p.stderr)]
    assert len(losses) >= 4
    assert losses[-1] < 0.7 * losses[0], losses
    assert "Train Done" in p.stdout
    ply = out + "_400.ply"
    assert os.path.exists(ply) and os.path.getsize(ply) > 20000 * 236
    # resume from the checkpoint (--load_itr, main.cpp:40-41)
    cmd2 = cmd[:]
    cmd2[cmd2.index("400")] = "450"
    p2 = subprocess.run(cmd2 + ["--load_itr", "400"], capture_output=True, text=True, timeout=600)
    assert p2.returncode == 0 and "(resumed)" in p2.stderr, p2.stderr
    assert os.path.exists(out + "_450.ply")
    # unknown flags are an error (CLI11 allow_config_extras(error), main.cpp:11); a dataset path is refused loudly
    assert subprocess.run([DRIVER, "--bogus", "1"], capture_output=True).returncode != 0
    p3 = subprocess.run([DRIVER, "--inputPath", "/nonexistent/dataset"], capture_output=True, text=True)
    assert p3.returncode != 0 and "load data failed" in p3.stdout


@pytest.mark.gpu
def test_cli_densify_prune_reset(tmp_path):
    """ADC active (SURVEY.md §8(f) row 1 / BASELINE config C5's "densify/prune active"): the splat count changes between
    iterations, training keeps going, the checkpoint has the new count and can be resumed."""
    out = str(tmp_path / "m" / "iteration")
    cmd = [DRIVER, "--inputPath", "synthetic:N=30000,W=320,H=240,cams=6,sh=2,seed=5", "--maxIteration", "1000", "--outputPath", out,
           "--warmupLength", "100", "--refineEvery", "100", "--resetAlphaEvery", "300", "--refineStopIter", "450", "--growGrad2d", "0.00005",
           "--densifyStrategy", "0"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    steps = [(int(m.group(1)), int(m.group(2)), int(m.group(3))) for m in re.finditer(r"densify @(\d+): (\d+) -> (\d+) splats", p.stderr)]
    assert len(steps) == 3 and steps[0][0] == 200, p.stderr[-1500:]        # refinement at 200, 300, 400 (stops before 450)
    assert any(b != a for _, a, b in steps)                      # the count really changes
    assert all(b <= 3_000_000 for _, _, b in steps)              # capacity = capMax (gs_train.cpp:89)
    losses = [float(m.group(2)) for m in re.finditer(r"Iteraions (\d+), loss : ([0-9.eE+-]+|nan|inf)", p.stderr)]
    # the opacity reset at 300 makes the loss jump (expected); by the end training has recovered
    assert len(losses) >= 9 and all(np.isfinite(losses)) and max(losses) > 0.3 and losses[-1] < 0.5 * losses[0]
    final_n = steps[-1][2]
    ply = out + "_1000.ply"
    assert os.path.getsize(ply) > final_n * 236 and os.path.getsize(ply) < final_n * 236 + 4096
    head = open(ply, "rb").read(400).decode(errors="ignore")
    assert f"element vertex {final_n}" in head
    p2 = subprocess.run(cmd[:cmd.index("1000")] + ["1020"] + cmd[cmd.index("1000") + 1:] + ["--load_itr", "1000"], capture_output=True, text=True, timeout=600)
    assert p2.returncode == 0 and "(resumed)" in p2.stderr, p2.stderr[-1500:]


@pytest.mark.gpu
def test_cli_mcmc_strategy(tmp_path):
    """--densifyStrategy 1 (MCMC, the CLI default: main.cpp:20,29): relocation + 5 % growth per interval up to the cap,
    exploration noise and the opacity/scale regularisers every step; training converges and the checkpoint has the new count."""
    out = str(tmp_path / "m" / "iteration")
    cmd = [DRIVER, "--inputPath", "synthetic:N=30000,W=320,H=240,cams=6,sh=2,seed=5", "--maxIteration", "800", "--outputPath", out,
           "--warmupLength", "100", "--refineEvery", "100", "--refineStopIter", "450", "--densifyStrategy", "1"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    steps = [(int(m.group(1)), int(m.group(2)), int(m.group(3))) for m in re.finditer(r"mcmc @(\d+): (\d+) -> (\d+) splats", p.stderr)]
    assert [s_[0] for s_ in steps] == [200, 300, 400], p.stderr[-1500:]
    n = 30000
    for _, a, b in steps:
        assert a == n and b == int(1.05 * a)
        n = b
    losses = [float(m.group(2)) for m in re.finditer(r"Iteraions (\d+), loss : ([0-9.eE+-]+|nan|inf)", p.stderr)]
    assert len(losses) >= 7 and all(np.isfinite(losses)) and losses[-1] < 0.6 * losses[0], losses
    head = open(out + "_800.ply", "rb").read(400).decode(errors="ignore")
    assert f"element vertex {n}" in head


@pytest.mark.gpu
def test_cli_adc_without_absgrad(tmp_path):
    """--densifyStrategy 0 --absgrad 0 (both exposed CLI flags): refinement must still happen — on hypot(gx W/2, gy H/2) of the signed
    dL/dmean2D, the standard rule (it used to be silently disabled). Which splats it picks on this non-square image is
    pinned by tests/test_train_step_options.py::test_plugin_adc_without_absgrad_uses_the_scaled_norm."""
    out = str(tmp_path / "m" / "iteration")
    cmd = [DRIVER, "--inputPath", "synthetic:N=20000,W=256,H=192,cams=4,sh=1,seed=7", "--maxIteration", "450", "--outputPath", out,
           "--warmupLength", "100", "--refineEvery", "100", "--refineStopIter", "400", "--growGrad2d", "0.00002", "--densifyStrategy", "0",
           "--absgrad", "0"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    steps = [(int(m.group(2)), int(m.group(3))) for m in re.finditer(r"densify @(\d+): (\d+) -> (\d+) splats", p.stderr)]
    assert len(steps) >= 2 and any(b > a for a, b in steps), p.stderr[-1500:]
    assert "useAbsGrad 0" in p.stderr


@pytest.mark.gpu
def test_cli_rccl_single_rank(tmp_path):
    """The plugin's data-parallel path (include/dvs_comm.h, librccl opened from C++) on the one GPU this box has: DVS_FORCE_COMM=1 runs
    the gradient exchange — both forms: factorised (all-gather of the colour gradients, all-reduce of the geometry groups, SH rows
    rebuilt with dvs_sh_grad_combine) and one all-reduce of all rows — and the statistics all-reduces of every step on a 1-rank RCCL
    communicator (the identity), so the runs must behave like the plain one: same refinement schedule and splat counts, same loss level."""
    import socket
    spec = ["--inputPath", "synthetic:N=20000,W=256,H=192,cams=4,sh=1,seed=7", "--maxIteration", "350", "--warmupLength", "100",
            "--refineEvery", "100", "--refineStopIter", "320", "--densifyStrategy", "1"]
    runs = []
    for force, exch in (("0", "factorised"), ("1", "factorised"), ("1", "allreduce")):
        s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
        env = dict(os.environ, DVS_FORCE_COMM=force, DVS_EXCHANGE=exch, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        p = subprocess.run([DRIVER] + spec + ["--outputPath", str(tmp_path / ("m" + force + exch) / "iteration")], capture_output=True, text=True,
                           timeout=600, env=env)
        assert p.returncode == 0, p.stdout + p.stderr
        counts = [int(m.group(3)) for m in re.finditer(r"mcmc @(\d+): (\d+) -> (\d+) splats", p.stderr)]
        losses = [float(m.group(2)) for m in re.finditer(r"Iteraions (\d+), loss : ([0-9.eE+-]+)", p.stderr)]
        runs.append((counts, losses, p.stderr))
    assert "RCCL communicator up" not in runs[0][2]
    assert "gradient exchange: factorised" in runs[1][2] and "gradient exchange: all-reduce of all rows" in runs[2][2]
    for k in (1, 2):
        assert runs[0][0] == runs[k][0] and len(runs[0][0]) == 2
        assert abs(runs[0][1][-1] - runs[k][1][-1]) < 0.05 * runs[0][1][-1], (runs[0][1], runs[k][1])


@pytest.mark.gpu
def test_cli_flags_mask_pack_prune(tmp_path):
    """Host flags the reference's CLI sets are honoured or named: --useMask (masked pixels carry no gradient), --packLevel 3
    (8-bit training views), --pruneStrategy / --pruneEvery (light prune after refinement stops), and the one-time report of
    ignored fields (--exportMesh). --minOpacity is accepted but, as in the reference host (gs_train.cpp:65 is commented out), never
    copied into the config: the prune threshold is the default 0.005, and on this rig it is the scale rule (0.1 x extent) that prunes."""
    out = str(tmp_path / "m" / "iteration")
    cmd = [DRIVER, "--inputPath", "synthetic:N=20000,W=256,H=192,cams=4,sh=1,seed=9", "--maxIteration", "420", "--outputPath", out,
           "--warmupLength", "50", "--refineEvery", "100", "--refineStopIter", "150", "--densifyStrategy", "0", "--useMask", "1",
           "--packLevel", "3", "--pruneStrategy", "1", "--pruneEvery", "200", "--minOpacity", "0.3", "--exportMesh", "1"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "PackF32ToU8: 8-bit training views" in p.stderr and "useMask 1" in p.stderr
    ign = [l for l in p.stderr.splitlines() if "IGNORED by this build:" in l]
    assert ign and "exportMesh" in ign[0] and "normalConsistencyLoss" in ign[0]
    prunes = [(int(m.group(1)), int(m.group(2)), int(m.group(3))) for m in re.finditer(r"light prune @(\d+): (\d+) -> (\d+) splats", p.stderr)]
    assert prunes and prunes[0][0] in (200, 400) and prunes[0][2] < prunes[0][1], p.stderr[-2000:]
    losses = [float(m.group(2)) for m in re.finditer(r"Iteraions (\d+), loss : ([0-9.eE+-]+|nan|inf)", p.stderr)]
    assert len(losses) >= 4 and all(np.isfinite(losses)) and max(losses) < 0.6     # (the light prune — opacity < 0.005 or scale > 0.1 x extent — and the mask keep it from falling)


@pytest.mark.gpu
def test_cli_c5_shape(tmp_path):
    """BASELINE config C5's shape through the plugin: 5M splats at 3840x2160, SH degree 3, densify / prune active, ~50 steps
    (HBM pressure: ~10 GB of parameters + moments, tile lists of ~10 M instances per view)."""
    out = str(tmp_path / "m" / "iteration")
    cmd = [DRIVER, "--inputPath", "synthetic:N=5000000,W=3840,H=2160,cams=2,sh=3,seed=2", "--maxIteration", "50", "--outputPath", out,
           "--warmupLength", "5", "--refineEvery", "20", "--refineStopIter", "45", "--densifyStrategy", "0", "--progressTrain", "0", "--ssim", "0.2"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    steps = [(int(m.group(1)), int(m.group(2)), int(m.group(3))) for m in re.finditer(r"densify @(\d+): (\d+) -> (\d+) splats", p.stderr)]
    assert [s_[0] for s_ in steps] == [20, 40] and all(0 < b <= 5_000_000 for _, _, b in steps), p.stderr[-2000:]
    assert "Train Done" in p.stdout
    head = open(out + "_50.ply", "rb").read(400).decode(errors="ignore")
    assert f"element vertex {steps[-1][2]}" in head


@pytest.mark.gpu
def test_cli_eight_views_per_iteration_as_one_pass(tmp_path):
    """BASELINE config C4 in the product: train_step renders 8 cameras per iteration as ONE multi-view pass (--viewsPerIter 8:
    dvs_raster_forward_views / the split backward over all views), gradients summed, one optimizer step. Reference run: the same eight
    cameras of every iteration one pass at a time with accumulating gradients (DVS_VIEWS_MODE=sequential). ADC refinement active in both
    (per-view abs-grad statistics). The two must take the same refinement decisions and follow the same loss trajectory."""
    def run(tag, env_extra):
        out = str(tmp_path / tag / "iteration")
        cmd = [DRIVER, "--inputPath", "synthetic:N=20000,W=320,H=240,cams=12,sh=2,seed=7", "--maxIteration", "500", "--outputPath", out,
               "--viewsPerIter", "8", "--densifyStrategy", "0", "--warmupLength", "100", "--refineEvery", "100", "--refineStopIter", "350",
               "--resetAlphaEvery", "3000", "--growGrad2d", "0.0004"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(os.environ, **env_extra))
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
        losses = [float(m.group(2)) for m in re.finditer(r"Iteraions (\d+), loss : ([0-9.eE+-]+)", p.stderr)]
        dens = [(int(m.group(1)), int(m.group(2)), int(m.group(3))) for m in re.finditer(r"densify @(\d+): (\d+) -> (\d+) splats", p.stderr)]
        return losses, dens, p.stderr
    lb, db, errb = run("batch", {})
    ls, ds, errs = run("seq", {"DVS_VIEWS_MODE": "sequential"})
    assert "ONE multi-view pass" in errb and "one pass per view" in errs
    assert len(lb) == len(ls) >= 5 and len(db) == len(ds) == 2, (lb, ls, db, ds)
    assert lb[-1] < 0.6 * lb[0], lb                                   # it trains
    for a, b in zip(lb[:3], ls[:3]):                                  # before the first refinement: the same trajectory to fp32 roundoff
        assert abs(a - b) <= 2e-3 * abs(b), (lb, ls)
    for a, b in zip(lb, ls):                                          # afterwards: the same level (refinement decisions sit on thresholds)
        assert abs(a - b) <= 0.05 * abs(b), (lb, ls)
    for (ia, na, ma), (ib, nb, mb) in zip(db, ds):                    # same schedule, counts within a per mille of each other
        assert ia == ib and na > 0 and abs(ma - mb) <= max(4, 0.002 * mb), (db, ds)
    # the environment override works for hosts that do not know the field
    out = str(tmp_path / "env" / "iteration")
    p = subprocess.run([DRIVER, "--inputPath", "synthetic:N=5000,W=160,H=96,cams=6,sh=1,seed=2", "--maxIteration", "20", "--outputPath", out],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, DVS_VIEWS_PER_ITER="4"))
    assert p.returncode == 0 and "4 views per trainStep" in p.stderr, p.stderr[-1500:]
