"""The plugin reads every extension variable once (ext_options.hpp read_env): a run with all twenty set to values outside their grammar
reports each exactly once, in the table's words, and writes byte for byte what a run with none of them set writes — every bad value left
its default. One save of a small synthetic scene with the mesh, the sky and the renders on, so that their rows are used too.

Two training runs of this trainer do not write the same bytes (its gradient sums are floating-point atomics: measured, two identical
5-step runs differ in the model and the sky texture in the last bits), so the two runs compared here train nothing: both resume a
model that a third run trained and saved (--load_itr with --maxIteration at the same step), and save once — a resumed save is
repeatable byte for byte. A bad value that leaked into what a save does would show: a PNG instead of a JPEG, a sky texture of another
size (it would not be read back), normals in the mesh header, an .lod / .transformed file."""
import os
import shutil
import subprocess
import pytest
from test_ext_options import ROWS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")
STEPS = 5
# one value per variable that its row refuses (tests/test_ext_options.py lists each among the row's refusals)
BAD = {
    "DVS_MESH_MIN_COMPONENT": "12.345", "DVS_MESH_NORMALS": "yes", "DVS_MESH_DECIMATE": "17", "DVS_MESH_BOUNDS": "0,0,0,inf,inf,inf", "DVS_MESH_TRUNC_VOXELS": "x",
    "DVS_RENDER_FORMAT": "bmp", "DVS_RENDER_LAYERS": "8", "DVS_RENDER_DEPTH_SCALE": "-5", "DVS_RENDER_PNG_LEVEL": "12", "DVS_EXPORT_LOD": "5", "DVS_LOD_RESOLUTION": "8",
    "DVS_MASK_CARVE": "0100", "DVS_SH_CULL_THRESHOLD": "nan", "DVS_REDUCED_HALF": "1x", "DVS_SKY_RESOLUTION": "abc", "DVS_SKY_LR": "0.05x",
    "DVS_FOCUS_REGION": "0,0,0,1,1,1x", "DVS_FOCUS_ROTATION": "nan,0,0", "DVS_EXPORT_TRANSFORM": "0,0,0,0,0,0,0", "DVS_EXPORT_ORIENT": "up",
}


def run(out, extra_env, *extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DVS_")}
    env.update(extra_env)
    p = subprocess.run([DRIVER, "--inputPath", "synthetic:N=2000,W=64,H=48,cams=3,sh=1,seed=4", "--maxIteration", str(STEPS), "--outputPath", out, "--meshResolution", "16",
                        "--exportMesh", "1", "--enableBg", "1", "--renderViews", "all"] + list(extra), capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    files = {}
    for d, _, names in os.walk(os.path.dirname(out)):
        for n in names:
            files[os.path.relpath(os.path.join(d, n), os.path.dirname(out))] = open(os.path.join(d, n), "rb").read()
    return files, p.stderr


def test_malformed_variables_are_each_reported_once_and_change_nothing(gpu_device, tmp_path):
    assert set(BAD) == set(ROWS) and all(BAD[var] in ROWS[var][4] for var in BAD)
    seed, _ = run(str(tmp_path / "seed" / "iteration"), {})
    for d in ("a", "b"):
        os.makedirs(tmp_path / d)
        for suffix in (".ply", ".sky"):
            shutil.copy(tmp_path / "seed" / f"iteration_{STEPS}{suffix}", tmp_path / d)
    plain, log_plain = run(str(tmp_path / "a" / "iteration"), {}, "--load_itr", str(STEPS))
    bad, log_bad = run(str(tmp_path / "b" / "iteration"), BAD, "--load_itr", str(STEPS))
    assert "(resumed" in log_plain and "(resumed" in log_bad and "sky: read the 256x128 texture" in log_plain and "sky: read the 256x128 texture" in log_bad
    for var, value in BAD.items():
        _, prefix, phrase, _, _ = ROWS[var]
        line = f"[gstrain] {prefix}: {var}='{value}' is not {phrase}: ignored"
        assert log_bad.splitlines().count(line) == 1 and log_bad.count(var + "=") == 1, (line, log_bad[-4000:])
        assert var + "=" not in log_plain, (var, log_plain[-4000:])
    names = {f"iteration_{STEPS}.ply", f"iteration_{STEPS}.sky", f"iteration_{STEPS}_mesh.ply"} | {f"iteration_{STEPS}_renders/cam_{c:04d}.jpg" for c in range(3)}
    assert set(seed) == names and set(plain) == names and set(bad) == names, (sorted(seed), sorted(plain), sorted(bad))
    assert plain[f"iteration_{STEPS}.ply"] == seed[f"iteration_{STEPS}.ply"] and plain[f"iteration_{STEPS}.sky"] == seed[f"iteration_{STEPS}.sky"]
    for name in sorted(names):
        assert plain[name] == bad[name] and len(plain[name]) > 0, name
