"""The extension options' table (divshot_amd/gstrain/ext_options.hpp): what each row accepts and refuses, through
gstrain_ext_option_check of libgsplyio.so under the variable's name and under the flag's, and through the built gaussian_train, which
refuses before the plugin is loaded. The accept / refuse columns below are written out by hand. For the rows with a flag they were
compared with the CLI of the commit before the table existed (acceptance there: no "Command Line Error"); the strings that CLI took and
the table refuses are PARENT_CLI_ACCEPTED — each was refused or silently dropped by the plugin, so the user got the default."""
import os
import subprocess
import pytest
from divshot_amd._lib import DvsError, ext_option_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "divshot_amd", "lib", "gaussian_train")

BOX = "x0,y0,z0,x1,y1,z1 with x1 > x0, y1 > y0, z1 > z0"
POSITIVE = "a finite number > 0"
# what no row takes (but the one that takes an infinite number): empty text, 4 KiB of digits, 1000 commas
DIGITS_4K = "9" * 4096
NEVER = ["", DIGITS_4K, "," * 1000]
BOX_YES = ["0,0,0,1,1,1", "-3,-2.5,2,3,2.5,8", "0,0,0,1e-3,1,1", "+0,0,0,+1,1,1"]
BOX_NO = ["0,0,0,0,1,1", "0,0,0,1,1,-1", "0,0,0,1,1", "0,0,0,1,1,1,1", "0,0,0,1,1,1x", "0,0,0,1,1,1,", "0,0,0,inf,inf,inf", "nan,0,0,1,1,1", "-inf,0,0,1,1,1"]
SWITCH_YES = ["0", "1"]
SWITCH_NO = ["2", "+1", "-1", "1x", "01", "yes", "true"]
RATE_YES = ["0.05", "4", "1e-3", "1e38", "+5"]
RATE_NO = ["0", "-1", "-0", "x", "0.05x", "nan", "inf", "1e60", "1e-60", "1,2"]

# variable: (flag or None, log prefix, phrase, accepted, refused) — the boundaries, one inside, one below, one above, a sign, trailing text,
# too many digits; nan and inf for the numbers; a wrong count for the comma lists
ROWS = {
    "DVS_MESH_MIN_COMPONENT": ("meshMinComponent", "mesh", "a percentage 0..100 with at most two decimals",
                               ["0", "100", "12.5", "12.50", "12.", "100.00", "007", "0.01"], ["100.01", "101", "+5", "-1", "5x", "1000", "12.345", ".5", "1e1", "12.5.1"]),
    "DVS_MESH_NORMALS": ("meshNormals", "mesh", "0 or 1", SWITCH_YES, SWITCH_NO),
    "DVS_MESH_DECIMATE": ("meshDecimate", "mesh", "0 (off) or an integer 2..16", ["0", "2", "16", "8", "02"], ["1", "17", "+2", "-2", "2x", "016", "2.0"]),
    "DVS_MESH_BOUNDS": (None, "mesh", BOX, BOX_YES, BOX_NO),
    "DVS_MESH_TRUNC_VOXELS": (None, "mesh", POSITIVE, RATE_YES, RATE_NO),
    "DVS_RENDER_FORMAT": ("renderFormat", "render", "jpg or png", ["jpg", "png"], ["bmp", "JPG", "jpg ", "jpg|png", "pn", "jpgx"]),
    "DVS_RENDER_LAYERS": (None, "render", "a sum 1..7 of 1 (color), 2 (depth), 4 (alpha)", ["1", "7", "3"], ["0", "8", "+3", "-1", "3x", "03", "color"]),
    "DVS_RENDER_DEPTH_SCALE": ("renderDepthScale", "render", POSITIVE, ["1000", "0.5", "1e-3", "1e38", "+5", "30000"], ["0", "-5", "-0", "12x", "nan", "inf", "1e60", "1e-60", "1,2"]),
    "DVS_RENDER_PNG_LEVEL": (None, "render", "a zlib level 0..9", ["0", "9", "6"], ["10", "12", "+6", "-1", "6x", "06"]),
    "DVS_EXPORT_LOD": ("exportLod", "lod", "a number of levels 0 (off) .. 4", ["0", "4", "2", "0004"], ["5", "+1", "-1", "1x", "00001", "two"]),
    "DVS_LOD_RESOLUTION": ("lodResolution", "lod", "a resolution 32..1024", ["32", "1024", "256", "0064"], ["31", "8", "1025", "+64", "-64", "64x", "00064"]),
    "DVS_MASK_CARVE": ("maskCarve", "mask carve", "a percentage 0 (off) .. 100", ["0", "100", "50", "050"], ["101", "+50", "-1", "50x", "0100", "fifty", "5.0"]),
    "DVS_SH_CULL_THRESHOLD": ("cullSHThreshold", "reduced", "a number >= 0", ["0", "0.01", "1e3", "+0.5", "-0", "inf", "1e60", DIGITS_4K], ["-0.01", "0.01x", "nan", "-inf", "1,2"]),
    "DVS_REDUCED_HALF": ("reducedHalf", "reduced", "0 or 1", SWITCH_YES, SWITCH_NO),
    "DVS_SKY_RESOLUTION": ("skyResolution", "sky", "a texture height (16..1024)", ["0", "99999", "128", "16", "1024", "00128"], ["+128", "-1", "128x", "100000", "abc", "12.5"]),
    "DVS_SKY_LR": (None, "sky", POSITIVE, RATE_YES, RATE_NO),
    "DVS_FOCUS_REGION": ("focusRegion", "focus region", BOX, BOX_YES, BOX_NO),
    "DVS_FOCUS_ROTATION": ("focusRotation", "focus region", "rx,ry,rz (radians)", ["0,0,0", "0.1,-0.2,3", "+0.1,0,0"], ["0,0", "0,0,0,0", "0,0,0x", "0,0,0,", "nan,0,0", "0,inf,0"]),
    "DVS_EXPORT_TRANSFORM": ("exportTransform", "exportTransform", "tx,ty,tz,rx,ry,rz,s with finite numbers and s > 0",
                             ["0,0,0,0,0,0,1", "0.5,-1,2,0.1,0.2,0.3,2.5", "0,0,0,0,0,0,1e-3"],
                             ["0,0,0,0,0,0", "0,0,0,0,0,0,0", "0,0,0,0,0,0,-1", "0,0,0,0,0,0,1,5", "0,0,0,0,0,0,1x", "nan,0,0,0,0,0,1", "0,0,0,0,0,0,inf"]),
    "DVS_EXPORT_ORIENT": ("exportOrient", "exportTransform", "one of +x -x +y -y +z -z", ["+x", "-x", "+y", "-y", "+z", "-z"], ["up", "y", "+w", "+yy", "++", "+Y"]),
}
# --renderLayers spells the sum of DVS_RENDER_LAYERS as names
LAYERS_FLAG = ("renderLayers", "color[,depth][,alpha]", {"color": 1, "color,depth": 3, "color,alpha": 5, "color,depth,alpha": 7},
               ["depth", "color,", ",color", "color,color", "color,alpha,depth", "colour", "3", "color,depth,alpha,color"])
# (flag, value): the CLI before the table accepted it, the table refuses it
PARENT_CLI_ACCEPTED = {("focusRegion", "0,0,0,inf,inf,inf"), ("focusRegion", "-inf,0,0,1,1,1"), ("focusRotation", "nan,0,0"), ("focusRotation", "0,inf,0")}


def flag_cases():
    """(flag, value, accepted) for every row with a flag"""
    for var, (flag, _, _, yes, no) in ROWS.items():
        if flag:
            for v in yes + no + never(yes):
                yield flag, v, v in yes
    for v in list(LAYERS_FLAG[2]) + LAYERS_FLAG[3] + NEVER:
        yield LAYERS_FLAG[0], v, v in LAYERS_FLAG[2]


def never(yes):
    return [v for v in NEVER if v not in yes]


def cli_message(flag, phrase, value):
    return f"Command Line Error: --{flag} takes {phrase}, not '{value}'"


def refusal(message):
    return (False, None, message[:1023])                                       # (the message buffer of ext_option_check: 1024 bytes)


@pytest.mark.parametrize("var", list(ROWS))
def test_a_row_takes_and_refuses_what_is_written_here_under_both_names(var):
    flag, prefix, phrase, yes, no = ROWS[var]
    for v in yes:
        ok, values, msg = ext_option_check(var, v)
        assert ok and msg == "" and len(values) == 8, (var, v, msg)
        if flag:
            assert ext_option_check(flag, v)[:2] == (True, values), (flag, v)
    for v in no + never(yes):
        assert ext_option_check(var, v) == refusal(f"{prefix}: {var}='{v}' is not {phrase}: ignored"), (var, v[:40])
        if flag:
            assert ext_option_check(flag, v) == refusal(cli_message(flag, phrase, v)), (flag, v[:40])


def test_the_layers_flag_is_translated_and_unknown_names_are_told_apart():
    flag, phrase, yes, no = LAYERS_FLAG
    for v, total in yes.items():
        ok, values, _ = ext_option_check(flag, v)
        assert ok and values[0] == total and ext_option_check("DVS_RENDER_LAYERS", str(total))[1] == values, v
    for v in no + NEVER:
        assert ext_option_check(flag, v) == refusal(cli_message(flag, phrase, v)), v[:40]
    for name in ("", "renderlayers", "--renderLayers", "DVS_RENDER_VIEWS", "meshResolution", "DVS_MESH_RESOLUTION"):
        with pytest.raises(DvsError):
            ext_option_check(name, "1")


def test_what_the_parsers_make_of_a_value():
    value = lambda name, text: ext_option_check(name, text)[1]
    assert [value("DVS_MESH_MIN_COMPONENT", t)[0] for t in ("12.5", "12.50", "12.", "007", "0.01", "100")] == [1250, 1250, 1200, 700, 1, 10000]
    assert value("meshDecimate", "02")[0] == 2 and value("DVS_SKY_RESOLUTION", "00128")[0] == 128 and value("DVS_REDUCED_HALF", "1")[0] == 1
    assert value("renderFormat", "jpg")[0] == 0 and value("renderFormat", "png")[0] == 1
    assert value("DVS_EXPORT_ORIENT", "-y")[:3] == [0.0, -1.0, 0.0] and value("exportOrient", "+z")[:3] == [0.0, 0.0, 1.0]
    assert value("focusRegion", "-3,-2.5,2,3,2.5,8")[:6] == [-3.0, -2.5, 2.0, 3.0, 2.5, 8.0]
    import numpy as np
    assert value("DVS_SKY_LR", "0.05")[0] == float(np.float32(0.05))               # numbers are read as float32, as the plugin keeps them
    assert value("exportTransform", "0.5,-1,2,0.1,0.2,0.3,2.5")[:7] == [float(np.float32(x)) for x in (0.5, -1, 2, 0.1, 0.2, 0.3, 2.5)]
    assert value("cullSHThreshold", "inf")[0] == float("inf")


def run_cli(*args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DVS_")}
    return subprocess.run([DRIVER] + list(args), capture_output=True, text=True, timeout=60, env=env)


def test_the_built_cli_refuses_with_the_rows_message_before_the_plugin_is_loaded():
    cases = [(flag, no[0], phrase) for flag, _, phrase, _, no in ROWS.values() if flag] + [(LAYERS_FLAG[0], LAYERS_FLAG[3][0], LAYERS_FLAG[1])]
    by_flag = {row[0]: row for row in ROWS.values() if row[0]}
    for flag, value in sorted(PARENT_CLI_ACCEPTED):                                # ... and what only the CLI used to take
        assert value in by_flag[flag][4]
        cases.append((flag, value, by_flag[flag][2]))
    assert len(cases) == 16 + 4
    for flag, value, phrase in cases:
        p = run_cli("--renderFormat", "png", f"--{flag}={value}") if flag != "renderFormat" else run_cli(f"--{flag}={value}")
        assert p.returncode == 1 and p.stdout == cli_message(flag, phrase, value) + "\n" and "gstrain" not in p.stderr, (flag, value, p.stdout, p.stderr)


def test_the_rules_across_options():
    for layers in ("color,depth", "color,alpha", "color,depth,alpha"):
        for fmt in ([], ["--renderFormat", "jpg"]):
            p = run_cli(*fmt, "--renderLayers", layers)
            assert p.returncode == 1 and p.stdout == ("Command Line Error: --renderLayers takes depth or alpha only with --renderFormat png (JPEG files carry colour alone), "
                                                      f"not '{layers}'\n"), (layers, fmt, p.stdout)
    p = run_cli("--exportTransform", "0,0,0,0,0,0,1", "--exportOrient", "+y")
    assert p.returncode == 1 and p.stdout == "Command Line Error: --exportTransform and --exportOrient exclude each other\n"
    for formats in ("transformed", "splat,transformed", "transformed,spz"):
        p = run_cli("--exportFormat", formats)
        assert p.returncode == 1 and p.stdout == "Command Line Error: --exportFormat transformed needs --exportTransform or --exportOrient\n", formats
    # none of the three is broken: the run gets as far as the plugin (which finds no device here, or trains there: either way no command line error)
    p = run_cli("--inputPath", "synthetic:N=0", "--renderFormat", "png", "--renderLayers", "color,depth", "--exportFormat", "transformed", "--exportOrient", "+y")
    assert "Command Line Error" not in p.stdout, p.stdout
