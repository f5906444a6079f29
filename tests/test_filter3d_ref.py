"""The 3D smoothing filter's restatement (tests/filter3d_ref.py) against itself, and the option's command line — no GPU:
  * chain is the transposed Jacobian of apply: central finite differences of apply in float64;
  * a zero filter is the identity of both;
  * the filter only ever blurs: effective opacity <= opacity, effective scale >= scale;
  * compute on a case small enough to read;
  * `--exportFormat fused` needs `--mipFilter3d 1`, and `--mipFilter3d 2` is refused with the table row's message before the plugin loads."""
import numpy as np
import filter3d_ref as F
from test_ext_options import run_cli, cli_message, refusal
from divshot_amd._lib import ext_option_check


def _inputs(n=400, seed=3):
    rng = np.random.default_rng(seed)
    scale = rng.uniform(-8, 2, (n, 3))
    opacity = rng.uniform(-12, 12, n)
    s = np.exp(scale.max(1))
    filt = np.concatenate([np.zeros(n // 4), 1e-3 * s[n // 4:n // 2], s[n // 2:3 * n // 4] * rng.uniform(0.5, 2, n // 4), 1e2 * s[3 * n // 4:]])
    return scale, opacity, filt, rng


def test_chain_is_the_transposed_jacobian_of_apply():
    scale, opacity, filt, rng = _inputs()
    n = opacity.size
    gs, go = rng.standard_normal((n, 3)), rng.standard_normal(n)
    cs, co = F.chain(scale, opacity, filt, gs, go)
    L = lambda s, a: (lambda se, oe: (se * gs).sum(1) + oe * go)(*F.apply(s, a, filt))      # per splat: the rows are independent
    h = 1e-5
    for k in range(3):
        d = np.zeros((n, 3)); d[:, k] = h
        fd = (L(scale + d, opacity) - L(scale - d, opacity)) / (2 * h)
        assert np.allclose(fd, cs[:, k], rtol=2e-6, atol=1e-8 * np.abs(cs).max()), (k, np.abs(fd - cs[:, k]).max())
    fd = (L(scale, opacity + h) - L(scale, opacity - h)) / (2 * h)
    assert np.allclose(fd, co, rtol=2e-6, atol=1e-8 * np.abs(co).max()), np.abs(fd - co).max()


def test_zero_filter_is_the_identity_bit_for_bit():
    scale, opacity, _, rng = _inputs()
    z = np.zeros(opacity.size)
    for dt in (np.float32, np.float64):
        s, a = scale.astype(dt), opacity.astype(dt)
        se, oe = F.apply(s, a, z, dt)
        assert se.dtype == dt and np.array_equal(se, s) and np.array_equal(oe, a)
        gs, go = rng.standard_normal(s.shape).astype(dt), rng.standard_normal(a.shape).astype(dt)
        cs, co = F.chain(s, a, z, gs, go, dt)
        assert np.array_equal(cs, gs) and np.array_equal(co, go)


def test_the_filter_only_blurs():
    scale, opacity, filt, _ = _inputs()
    se, oe = F.apply(scale, opacity, filt)
    on = filt > 0
    assert np.all(se[on] > scale[on]) and np.all(oe[on] < opacity[on]) and np.all(np.isfinite(oe)) and np.all(np.isfinite(se))
    # far above the scales the splat becomes the filter itself; far below nothing changes
    far = slice(3 * opacity.size // 4, None)
    assert np.allclose(np.exp(se[far]), filt[far, None], rtol=1e-3)
    near = slice(opacity.size // 4, opacity.size // 2)
    assert np.allclose(se[near].max(1), scale[near].max(1), atol=1e-6)
    # a = +-20 stays finite in float32 too
    a = np.array([-20, 20, -20, 20], np.float32)
    s = np.full((4, 3), -3, np.float32)
    f = np.array([1e-3, 1e-3, 10, 10], np.float32)
    assert np.all(np.isfinite(F.apply(s, a, f, np.float32)[1]))


class _Cam:
    def __init__(self, x, f, w, h):
        self.view = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -x, 0, 0, 1]           # view[c*4+r]: camera at (x, 0, 0) looking down +z
        self.focal_x, self.width, self.height = f, w, h


def test_compute_on_a_case_small_enough_to_read():
    rows = F.pack_cameras([_Cam(0, 100, 64, 48), _Cam(1, 50, 64, 48)])
    assert rows.shape == (2, 16) and list(rows[1, :4]) == [1, 0, 0, -1] and list(rows[1, 12:]) == [50, 64, 48, 0]
    pos = np.array([[0, 0, 2], [1, 0, 1], [0, 0, 0.1], [0, 100, 2], [np.nan, 0, 2], [0.5, 0, 4]])
    filt, seen = F.compute(pos, rows)
    # splat 0: camera 0 at z 2 (2/100), camera 1 sees it too (|(-1)/2 * 50| = 25 <= 41.6: 2/50): min 0.02; splat 1: camera 1 alone (x/z f = 100 for camera 0)
    assert list(seen) == [True, True, False, False, False, True]
    r = np.sqrt(0.2)
    assert np.allclose(filt, [r * 0.02, r * 0.02, r * 0.04, r * 0.04, r * 0.04, r * 0.04])
    none, seen = F.compute(pos[2:5], rows)
    assert not seen.any() and np.array_equal(none, np.zeros(3))


def test_the_cli_knows_the_option_and_what_fused_needs():
    phrase = "0 or 1"
    assert ext_option_check("DVS_MIP_FILTER3D", "1")[:2] == (True, [1.0] + [0.0] * 7) and ext_option_check("mipFilter3d", "0")[0]
    assert ext_option_check("DVS_MIP_FILTER3D", "2") == refusal(f"filter3d: DVS_MIP_FILTER3D='2' is not {phrase}: ignored")
    for bad in ("2", "", "01", "yes"):
        p = run_cli(f"--mipFilter3d={bad}")
        assert p.returncode == 1 and p.stdout == cli_message("mipFilter3d", phrase, bad) + "\n" and "gstrain" not in p.stderr, (bad, p.stdout, p.stderr)
    for args in (["--exportFormat", "fused"], ["--exportFormat", "splat,fused"], ["--exportFormat", "fused", "--mipFilter3d", "0"]):
        p = run_cli(*args)
        assert p.returncode == 1 and p.stdout == "Command Line Error: --exportFormat fused needs --mipFilter3d 1\n" and "gstrain" not in p.stderr, (args, p.stdout)
    # with the filter on the token is taken: the run gets as far as the plugin (no device here, or a refused scene there: no command line error)
    p = run_cli("--inputPath", "synthetic:N=0", "--mipFilter3d", "1", "--exportFormat", "fused,splat")
    assert "Command Line Error" not in p.stdout, p.stdout
