"""The training-side kernels (densify.hip, mcmc.hip, ssim.hip, train_ops.hip) at the sizes the product
runs them: across the chunk boundary of the single-workgroup block-sum scans (n > 65 536), at 10^6 splats, at 1920x1080, and at
the degenerate edges. Every reference is fp64 numpy restated from the rule in include/dvs_train.h, every check is vectorised."""
import ctypes as C
import numpy as np
import pytest
from util import gauss_window, conv_same, relocation_np, rel_close
from densify_ref import capped as _capped_want      # the documented cap, restated once (tests/densify_ref.py)

pytestmark = pytest.mark.gpu

KEEP, CLONE, SPLIT, PRUNE = 0, 1, 2, 3
SSIM_C1, SSIM_C2 = 0.01 ** 2, 0.03 ** 2


def _st():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sig(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def _excl_cumsum(c):
    return np.concatenate([[0], np.cumsum(c, dtype=np.int64)[:-1]]) if len(c) else np.zeros(0, np.int64)


def _quat_rot_np(q):
    """rotation matrices [n,3,3] of (w,x,y,z) quaternions, normalised (fp64)"""
    q = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)


# ---------------------------------------------------------------------------------------------------------------------------
# 1-2. ADC plan / apply
# ---------------------------------------------------------------------------------------------------------------------------
def _adc_scene(n, seed):
    """splat arrays whose rot[:, 3] is the exact splat id (copied verbatim by every action), and interval statistics. Runs of
    pruned splats over block and chunk boundaries, a pruned last splat, and a block of growth candidates at the start."""
    rng = np.random.default_rng(seed)
    A = {"pos": rng.normal(size=(n, 3)), "sh0": rng.normal(size=(n, 3)), "shN": rng.normal(size=(n, 15, 3)),
         "opacity": rng.normal(0, 3, size=(n,)), "scale": rng.normal(-3, 1, size=(n, 3)), "rot": rng.normal(size=(n, 4))}
    A = {k: v.astype(np.float32) for k, v in A.items()}
    A["rot"][:, 3] = np.arange(n, dtype=np.float32)              # exact below 2^24
    for lo, hi in ((200, 300), (65_500, 65_600), (n - 70, n)):   # dead runs across block / chunk boundaries, dead last splat
        A["opacity"][max(lo, 0):min(hi, n)] = -9.0
    denom = rng.integers(0, 6, n).astype(np.float32)
    avg = np.abs(rng.normal(0, 2.5e-4, n))
    avg[:150] = 1e-3                                             # growth inside the first block
    ga = (avg * denom).astype(np.float32)
    mr = rng.integers(0, 40, n).astype(np.int32)
    return A, ga, denom, mr


def _adc_want(A, ga, de, mr, grad_thr, scale_thr, min_op):
    sig = _sig(A["opacity"])
    smax = np.exp(A["scale"].max(1).astype(np.float64))
    avg = np.where(de > 0, ga.astype(np.float64) / np.maximum(de, 1), 0.0)
    want = np.where(sig < min_op, PRUNE, np.where(avg >= grad_thr, np.where(smax > scale_thr, SPLIT, CLONE), KEEP))
    borderline = (np.abs(sig - min_op) < 1e-6) | (np.abs(avg - grad_thr) < 1e-6 * grad_thr) | (np.abs(smax - scale_thr) < 1e-6)
    return want, borderline


class _Adc:
    """device copies of an ADC scene and the plan / apply calls"""

    def __init__(self, A, ga, de, mr, tiled, dev):
        import torch
        from divshot_amd.raster import shn_rows_to_tiled_np
        self.n, self.A, self.tiled, self.dev = len(ga), A, tiled, dev
        t = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
        self.ga, self.de, self.mr = t(ga), t(de), t(mr)
        shn = shn_rows_to_tiled_np(A["shN"]) if tiled else A["shN"].reshape(-1)
        self.src = [t(A["pos"].reshape(-1)), t(A["sh0"].reshape(-1)), t(shn), t(A["opacity"]), t(A["scale"].reshape(-1)), t(A["rot"].reshape(-1))]
        n = self.n
        self.action = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.offs = torch.zeros(n, dtype=torch.int32, device=dev)
        self.scratch = torch.zeros(n // 256 + 2, dtype=torch.int32, device=dev)      # exactly the documented minimum
        self.total = torch.zeros(1, dtype=torch.int64, device=dev)

    def plan(self, prm):
        import torch
        from divshot_amd._lib import lib, check
        check(lib.dvs_densify_plan(_st(), self.n, self.src[3].data_ptr(), self.src[4].data_ptr(), self.ga.data_ptr(), self.de.data_ptr(),
                                   self.mr.data_ptr(), C.byref(prm), self.action.data_ptr(), self.offs.data_ptr(), self.scratch.data_ptr(),
                                   self.total.data_ptr()), "dvs_densify_plan")
        torch.cuda.synchronize()
        return self.action.cpu().numpy().copy(), self.offs.cpu().numpy().view(np.uint32).astype(np.int64), int(self.total.item())

    def apply(self, prm, mode, new_n):
        """-> the six destination arrays as host rows (shN [new_n,15,3]); destinations start as NaN"""
        import torch
        from divshot_amd._lib import lib, check
        from divshot_amd.raster import tiled_floats, shn_tiled_to_rows_np
        dev = self.dev
        sizes = [new_n * 3, new_n * 3, tiled_floats(new_n) if self.tiled else new_n * 45, new_n, new_n * 3, new_n * 4]
        dst = [torch.full((s,), float("nan"), device=dev) for s in sizes]
        sp = (C.c_void_p * 6)(*[x.data_ptr() for x in self.src]); dp = (C.c_void_p * 6)(*[x.data_ptr() for x in dst])
        check(lib.dvs_densify_apply(_st(), self.n, self.action.data_ptr(), self.offs.data_ptr(), C.byref(prm), mode, sp, dp, new_n),
              "dvs_densify_apply")
        torch.cuda.synchronize()
        h = [x.cpu().numpy() for x in dst]
        shn = shn_tiled_to_rows_np(h[2], new_n) if self.tiled else h[2].reshape(new_n, 15, 3)
        return {"pos": h[0].reshape(new_n, 3), "sh0": h[1].reshape(new_n, 3), "shN": shn, "opacity": h[3],
                "scale": h[4].reshape(new_n, 3), "rot": h[5].reshape(new_n, 4)}


def _check_apply(A, act, offs, new_n, out, mode):
    """row-by-row check of one dvs_densify_apply result against numpy gathers of the source rows"""
    n = len(act)
    cnt = np.where(act == PRUNE, 0, np.where(act == KEEP, 1, 2))
    src = np.repeat(np.arange(n), cnt)                               # source splat of every output row
    assert src.size == new_n
    copy = np.arange(new_n) - offs[src]                              # 0 or 1: which result of its source
    a = act[src]
    verbatim = (a == KEEP) | ((a == CLONE) & (copy == 0)) | ((a == CLONE) & (mode == 0))
    if mode == 0:
        assert np.array_equal(out["rot"][:, 3], src.astype(np.float32)), "output rows do not decode to the planned sources"
        for k in ("pos", "sh0", "shN", "opacity", "scale", "rot"):
            assert np.array_equal(out[k][verbatim], A[k][src[verbatim]]), k
        sp = a == SPLIT
        for k in ("sh0", "shN", "opacity", "rot"):
            assert np.array_equal(out[k][sp], A[k][src[sp]]), k
        np.testing.assert_allclose(out["scale"][sp], A["scale"][src[sp]] - np.log(1.6), rtol=0, atol=2e-6)
        # children = pos + R diag(exp s) z, z ~ N(0, I) by Box-Muller from 24-bit uniforms: |z_k| <= sqrt(-2 ln 2^-25) < 5.9
        R = _quat_rot_np(A["rot"][src[sp]])
        z = np.einsum("nji,nj->ni", R, out["pos"][sp].astype(np.float64) - A["pos"][src[sp]]) / np.exp(A["scale"][src[sp]].astype(np.float64))
        assert not sp.any() or np.abs(z).max() < 5.9 + 1e-3, np.abs(z).max()
        if sp.sum() > 3000:                                          # sample moments of z: unit normal
            assert abs(z.mean()) < 0.05 and abs(z.var() - 1.0) < 0.05, (z.mean(), z.var())
        first = sp & (copy == 0)
        assert not (out["pos"][first] == out["pos"][np.nonzero(first)[0] + 1]).all(1).any()      # the two children differ
    else:
        for k in ("pos", "sh0", "shN", "opacity", "scale", "rot"):
            assert np.array_equal(out[k][verbatim], A[k][src[verbatim]]), k
            assert not out[k][~verbatim].any(), k                   # moments of new splats are zero


@pytest.mark.parametrize("n,tiled", [(65_536, False), (65_537, True), (65_536 + 255, False), (1_000_003, False), (1_000_003, True)])
def test_densify_plan_apply_across_scan_chunks(gpu_device, n, tiled):
    """dvs_densify_plan / dvs_densify_apply where the block-sum scan carries between chunks of 256 blocks (n > 65 536; 1 000 003 splats
    = 3 907 blocks = 16 chunks): action against the rule, offsets / new count exactly the scan of the GPU's own actions, every
    output row of both modes against numpy gathers."""
    from divshot_amd._lib import DensifyParams
    A, ga, de, mr = _adc_scene(n, seed=n % 1000)
    prm = DensifyParams(grad_threshold=2e-4, scale_threshold=0.05, min_opacity=0.005, max_world_scale=0.0, max_screen_radius=0,
                        cap_max=0, seed=91, shn_layout=int(tiled))
    d = _Adc(A, ga, de, mr, tiled, gpu_device)
    act, offs, new_n = d.plan(prm)
    want, borderline = _adc_want(A, ga, de, mr, 2e-4, 0.05, 0.005)
    assert np.array_equal(act[~borderline], want[~borderline])
    assert {KEEP, CLONE, SPLIT, PRUNE} <= set(np.unique(act).tolist()) and act[-1] == PRUNE
    cnt = np.where(act == PRUNE, 0, np.where(act == KEEP, 1, 2))
    assert np.array_equal(offs, _excl_cumsum(cnt)) and new_n == int(cnt.sum())
    for mode in (0, 1):
        _check_apply(A, act, offs, new_n, d.apply(prm, mode, new_n), mode)


def test_densify_cap_max(gpu_device):
    """include/dvs_train.h: growth is cut off deterministically by splat index at cap_max. Cut points inside the first block, inside a
    middle chunk of the block-sum scan, exactly at the uncapped count, at the survivor count and below it; PRUNE never changes,
    the demoted candidates are those of highest index, new_count = min(uncapped, max(cap_max, survivors)), offsets are the scan of
    the final actions and apply writes every surviving splat."""
    from divshot_amd._lib import DensifyParams
    n = 200_003                                                     # 782 blocks: 4 chunks of the block-sum scan
    A, ga, de, mr = _adc_scene(n, seed=5)
    prm = DensifyParams(grad_threshold=2e-4, scale_threshold=0.05, min_opacity=0.005, max_world_scale=0.0, max_screen_radius=0,
                        cap_max=0, seed=17, shn_layout=1)
    d = _Adc(A, ga, de, mr, True, gpu_device)
    act0, offs0, uncapped = d.plan(prm)
    grow = np.nonzero((act0 == CLONE) | (act0 == SPLIT))[0]
    S = int((act0 != PRUNE).sum())
    assert uncapped == S + len(grow) and grow[0] < 256 and len(grow) > 1000
    g_first_block = int((grow < 256).sum())
    g_mid = int((grow < 150_000).sum())                             # block 585, third chunk
    cuts = {"first block": S + g_first_block // 2, "middle chunk": S + g_mid, "uncapped": uncapped, "survivors": S,
            "below survivors": S - 1000, "one": 1}
    for name, cap in cuts.items():
        prm.cap_max = cap
        act, offs, new_n = d.plan(prm)
        want, _, _ = _capped_want(act0, cap)
        assert np.array_equal(act == PRUNE, act0 == PRUNE), name
        assert np.array_equal(act, want), (name, int((act != want).sum()))
        assert new_n == min(uncapped, max(cap, S)), (name, new_n, cap, S, uncapped)
        cnt = np.where(act == PRUNE, 0, np.where(act == KEEP, 1, 2))
        assert np.array_equal(offs, _excl_cumsum(cnt)) and new_n == int(cnt.sum()), name
        if name in ("middle chunk", "below survivors"):
            _check_apply(A, act, offs, new_n, d.apply(prm, 0, new_n), 0)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. multi-view statistics (dvs_densify_accumulate_rows, dvs_any_view_radius)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [8, 1])
def test_densify_accumulate_rows_multi_view(gpu_device, V):
    """The ADC statistics of a multi-view pass, read from the A8 rows between backward_composite and backward_project (the plugin's
    order), on top of nonzero statistics == V single-view passes each followed by dvs_densify_accumulate on its absgrad2d. One view
    sees nothing. denom / max_radii exact, grad_accum at the A8 bar; dvs_any_view_radius == max over the views."""
    import torch
    import divshot_amd as dv
    from divshot_amd._lib import lib, check, FwdState
    from divshot_amd.raster import Rasterizer, params_to_device
    n, W, H = 20_011, 176, 112
    spec = dv.make_spec(n, W, H, sh_degree=2, n_cams=max(V, 2), seed=31)
    P = dv.synth_splats(spec)
    cams = [dv.synth_camera(spec, v) for v in range(V)]
    if V > 1:
        for c in range(4):
            cams[3].view[c * 4 + 2] = -cams[3].view[c * 4 + 2]     # view 3 looks the other way: culled entirely
    tg = [torch.from_numpy(dv.synth_target(spec, v)).to(gpu_device) for v in range(V)]
    rng = np.random.default_rng(V)
    ga0 = rng.random(n).astype(np.float32) * 1e-3
    de0 = rng.integers(0, 4, n).astype(np.float32)
    mr0 = rng.integers(0, 30, n).astype(np.int32)
    t = lambda a: torch.tensor(a, device=gpu_device)
    st = _st()

    single = Rasterizer(0, max_splats=n, max_w=W, max_h=H)
    Pd = params_to_device(P, single.tdev)
    ga, de, mr = t(ga0), t(de0), t(mr0)
    radii_single = []
    for v in range(V):
        img = single.forward(Pd, cams[v], sh_degree=2, absgrad=True)
        g = single.backward(((img - tg[v]) / (W * H)).contiguous())
        radii = t(single.saved()["radii"])
        radii_single.append(radii.cpu().numpy())
        check(lib.dvs_densify_accumulate(st, n, radii.data_ptr(), g["absgrad2d"].data_ptr(), W, H, ga.data_ptr(), de.data_ptr(), mr.data_ptr()))
    torch.cuda.synchronize()
    radii_single = np.stack(radii_single)
    if V > 1:
        assert (radii_single[3] == 0).all() and all((radii_single[v] > 0).any() for v in range(V) if v != 3)
        assert any(not np.array_equal(radii_single[0] > 0, radii_single[v] > 0) for v in (1, 2, 4, 5, 6, 7))   # different subsets

    batch = Rasterizer(0, max_splats=n, max_w=W, max_h=H, max_views=V)
    imgs = batch.forward_views(Pd, cams, sh_degree=2, absgrad=True)
    dL = torch.stack([(imgs[v] - tg[v]) / (W * H) for v in range(V)]).contiguous()
    batch.backward_composite(dL)
    rows, rf = C.c_void_p(), C.c_int(0)
    check(lib.dvs_get_bwd_intermediates(batch.ctx, C.byref(rows), C.byref(rf)))
    assert rf.value == 12
    fs = FwdState()
    check(lib.dvs_get_view_state(batch.ctx, 0, C.byref(fs)))       # radii of the batch: [V][n] from view 0's pointer
    gb, db, mb = t(ga0), t(de0), t(mr0)
    check(lib.dvs_densify_accumulate_rows(st, n, V, fs.radii, rows.value, W, H, gb.data_ptr(), db.data_ptr(), mb.data_ptr()))
    anyr = torch.full((n,), -1, dtype=torch.int32, device=gpu_device)
    check(lib.dvs_any_view_radius(st, n, V, fs.radii, anyr.data_ptr()))
    batch.backward_project()
    torch.cuda.synchronize()
    radii_batch = batch._d2h(fs.radii, (V, n), np.int32)
    assert np.array_equal(radii_batch, radii_single)
    assert np.array_equal(db.cpu().numpy(), de.cpu().numpy())
    assert np.array_equal(mb.cpu().numpy(), mr.cpu().numpy())
    ok, worst = rel_close(gb.cpu().numpy(), ga.cpu().numpy(), 1e-4, 2e-6)
    assert ok.all(), worst
    assert np.array_equal(anyr.cpu().numpy(), radii_single.max(0))
    # the statistics moved where some view saw the splat, and only there
    seen = (radii_single > 0).any(0)
    assert np.array_equal(db.cpu().numpy() != de0, seen)
    single.close(); batch.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. MCMC at scale
# ---------------------------------------------------------------------------------------------------------------------------
_MCMC_W = [3, 3, 45, 1, 3, 4]


class _Mcmc:
    def __init__(self, P, n, cap, tiled, dev):
        import torch
        from divshot_amd._lib import lib, check, McmcSets
        from divshot_amd.raster import shn_rows_to_tiled_np
        self.n, self.cap, self.tiled, self.dev = n, cap, tiled, dev
        self.par = []
        for g, w in enumerate(_MCMC_W):
            full = np.zeros((cap, w), np.float32); full[:n] = P[g]
            self.par.append(torch.tensor(shn_rows_to_tiled_np(full) if (g == 2 and tiled) else full.reshape(-1), device=dev))
        self.mom = [[torch.ones_like(p) for p in self.par] for _ in range(2)]
        self.sets = McmcSets()
        for g in range(6):
            self.sets.param[g], self.sets.m[g], self.sets.v[g] = self.par[g].data_ptr(), self.mom[0][g].data_ptr(), self.mom[1][g].data_ptr()
        self.scratch = torch.empty(int(lib.dvs_mcmc_scratch_bytes(cap)), dtype=torch.uint8, device=dev)
        check(lib.dvs_mcmc_init_scratch(_st(), self.scratch.data_ptr(), cap))

    def host(self, t, g):
        from divshot_amd.raster import shn_tiled_to_rows_np
        a = t.cpu().numpy()
        return shn_tiled_to_rows_np(a, self.cap).reshape(self.cap, 45) if (g == 2 and self.tiled) else a.reshape(self.cap, _MCMC_W[g])

    def params(self):
        return [self.host(self.par[g], g) for g in range(6)]

    def moments(self):
        return [[self.host(mm[g], g) for g in range(6)] for mm in self.mom]


def _check_draws(P0, P1, M1, dst, srcs, n, min_op, touched_extra=()):
    """dst rows are copies of srcs (live); every drawn splat and its copies carry the relocated opacity / scale; everything else in
    [0, n) is bit-identical; moments of touched rows are zero, the rest untouched (1)."""
    o0 = _sig(P0[3][:n, 0])
    assert not (o0[srcs] <= min_op).any(), "a dead splat was drawn"
    for g in (0, 1, 2, 5):
        assert np.array_equal(P1[g][dst], P0[g][srcs]), g
    cnt = np.bincount(srcs, minlength=n)
    drawn = np.nonzero(cnt)[0]
    rows = np.concatenate([drawn, dst]); src_of = np.concatenate([drawn, srcs])
    ratio = cnt[src_of] + 1
    want_o = np.empty(rows.size); want_ls = np.empty(rows.size)
    for r in np.unique(ratio):
        sel = ratio == r
        no, coeff = relocation_np(o0[src_of[sel]], int(min(r, 51)), min_op)
        want_o[sel], want_ls[sel] = no, np.log(coeff)
    got_o = _sig(P1[3][rows, 0])
    assert (np.abs(got_o - want_o) <= 2e-5 * np.maximum(want_o, 1e-3)).all(), np.abs(got_o - want_o).max()
    np.testing.assert_allclose(P1[4][rows], P0[4][src_of] + want_ls[:, None], rtol=0, atol=3e-5)
    touched = np.zeros(P1[0].shape[0], bool); touched[rows] = True; touched[list(touched_extra)] = True
    untouched = ~touched[:n]
    for g in range(6):
        assert np.array_equal(P1[g][:n][untouched], P0[g][:n][untouched]), g
        for M in M1:
            assert (M[g][touched] == 0).all() and (M[g][:n][untouched] == 1).all(), g
    return cnt


def _chi2_opacity_bins(o_live, draws_per_splat, bins=10):
    """chi-square of the per-bin draw counts (splats binned by opacity quantile) against draws proportional to opacity"""
    edges = np.quantile(o_live, np.linspace(0, 1, bins + 1))
    b = np.clip(np.searchsorted(edges, o_live, side="right") - 1, 0, bins - 1)
    got = np.bincount(b, weights=draws_per_splat, minlength=bins)
    want = draws_per_splat.sum() * np.bincount(b, weights=o_live, minlength=bins) / o_live.sum()
    return float(((got - want) ** 2 / want).sum())


CHI2_9DOF_P001 = 27.88                                             # 0.999 quantile of chi-square with 9 degrees of freedom


@pytest.mark.parametrize("tiled", [False, True])
def test_mcmc_relocate_grow_at_scale(gpu_device, tiled):
    """dvs_mcmc_relocate / dvs_mcmc_grow at 200 000 splats, capacity 260 000 (782 blocks: 4 chunks of the block-sum scan), ~10 %
    dead including runs across block and chunk boundaries and the last splat: destinations = the dead set exactly, sources live,
    relocated opacity / scale of every drawn splat and copy, untouched rows bit-identical, draws proportional to opacity."""
    import torch
    from divshot_amd._lib import lib, check
    rng = np.random.default_rng(21 + tiled)
    n, cap, n_new, min_op = 200_000, 260_000, 10_000, 0.005
    P = [rng.standard_normal((n, w)).astype(np.float32) for w in _MCMC_W]
    P[5][:, 3] = np.arange(n)                                       # rot[:, 3] = splat id: copied verbatim, exact below 2^24
    P[3][:, 0] = rng.normal(0, 2.0, n)
    dead = rng.random(n) < 0.09
    for lo, hi in ((250, 300), (65_530, 65_560), (131_000, 131_100), (n - 40, n)):
        dead[lo:hi] = True
    P[3][dead, 0] = -8.0
    P[4] = rng.normal(-3, 0.3, (n, 3)).astype(np.float32)
    dead = _sig(P[3][:, 0]) <= min_op
    m = _Mcmc(P, n, cap, tiled, gpu_device)
    P0 = m.params()
    n_dead = torch.zeros(1, dtype=torch.int32).pin_memory()
    check(lib.dvs_mcmc_relocate(_st(), n, C.byref(m.sets), min_op, 7, int(tiled), m.scratch.data_ptr(), cap, n_dead.data_ptr()), "relocate")
    torch.cuda.synchronize()
    assert int(n_dead[0]) == int(dead.sum())
    P1, M1 = m.params(), m.moments()
    ids = P1[5][:n, 3].astype(np.int64)
    dst = np.nonzero(ids != np.arange(n))[0]
    assert np.array_equal(dst, np.nonzero(dead)[0]), "destinations are not the dead set"
    srcs = ids[dst]
    cnt = _check_draws(P0, P1, M1, dst, srcs, n, min_op)
    live = ~dead
    chi2 = _chi2_opacity_bins(_sig(P[3][live, 0]), cnt[live])
    assert chi2 < CHI2_9DOF_P001, chi2
    assert (P1[0][n:] == 0).all()
    # grow: re-stamp the ids (relocated copies share their source's), moments back to 1
    m.par[5].view(cap, 4)[:n, 3] = torch.arange(n, dtype=torch.float32, device=gpu_device)
    for mm in m.mom:
        for x in mm:
            x.fill_(1.0)
    P1 = m.params()
    check(lib.dvs_mcmc_grow(_st(), n, n_new, C.byref(m.sets), min_op, 8, int(tiled), m.scratch.data_ptr(), cap), "grow")
    torch.cuda.synchronize()
    P2, M2 = m.params(), m.moments()
    new_rows = np.arange(n, n + n_new)
    srcs2 = P2[5][new_rows, 3].astype(np.int64)
    cnt2 = _check_draws(P1, P2, M2, new_rows, srcs2, n, min_op)
    live1 = _sig(P1[3][:n, 0]) > min_op
    chi2 = _chi2_opacity_bins(_sig(P1[3][:n, 0])[live1], cnt2[live1])
    assert chi2 < CHI2_9DOF_P001, chi2
    assert (P2[0][n + n_new:] == 0).all() and all((M[g][n + n_new:] == 1).all() for M in M2 for g in range(6))


def test_mcmc_noise_and_regularizer_ranges(gpu_device):
    """dvs_mcmc_add_noise_range / dvs_mcmc_regularize_range over an uneven partition of [0, n) == the whole-array launches, bit for
    bit (the plugin's pipelined exchange launches them per chunk). A launch on chunk-relative pointers (chunk-local indices) must not
    be: that is what the comparison would see if the range launch drew its numbers from the local index."""
    import torch
    from divshot_amd._lib import lib, check
    n = 200_000
    rng = np.random.default_rng(9)
    pos = rng.normal(size=(n, 3)).astype(np.float32)
    scale = rng.normal(-3, 0.5, (n, 3)).astype(np.float32)
    rot = rng.normal(size=(n, 4)).astype(np.float32)
    opa = rng.normal(-4, 3, n).astype(np.float32)                  # a good share of faint splats: the noise gate is open
    t = lambda a: torch.tensor(a, device=gpu_device)
    ds, dr, do = t(scale), t(rot), t(opa)
    st = _st()
    chunks = [(0, 1), (1, 256), (257, 65_280), (65_537, 70_000), (135_537, 64_463)]
    assert sum(c for _, c in chunks) == n and all(chunks[k][0] + chunks[k][1] == chunks[k + 1][0] for k in range(len(chunks) - 1))
    whole, ranged, local = t(pos), t(pos), t(pos)
    check(lib.dvs_mcmc_add_noise(st, n, whole.data_ptr(), ds.data_ptr(), dr.data_ptr(), do.data_ptr(), 0.3, 1234))
    for f, c in chunks:
        check(lib.dvs_mcmc_add_noise_range(st, n, f, c, ranged.data_ptr(), ds.data_ptr(), dr.data_ptr(), do.data_ptr(), 0.3, 1234))
        check(lib.dvs_mcmc_add_noise_range(st, c, 0, c, local.data_ptr() + 12 * f, ds.data_ptr() + 12 * f, dr.data_ptr() + 16 * f,
                                           do.data_ptr() + 4 * f, 0.3, 1234))
    torch.cuda.synchronize()
    moved = (whole != t(pos)).any(1)
    assert moved.float().mean() > 0.3
    assert torch.equal(ranged, whole)
    assert not torch.equal(local[chunks[2][0]:], whole[chunks[2][0]:])
    go0 = rng.normal(size=n).astype(np.float32); gs0 = rng.normal(size=(n, 3)).astype(np.float32)
    gow, gsw, gor, gsr = t(go0), t(gs0), t(go0), t(gs0)
    check(lib.dvs_mcmc_regularize(st, n, do.data_ptr(), ds.data_ptr(), gow.data_ptr(), gsw.data_ptr(), 0.01, 0.02))
    for f, c in chunks:
        check(lib.dvs_mcmc_regularize_range(st, n, f, c, do.data_ptr(), ds.data_ptr(), gor.data_ptr(), gsr.data_ptr(), 0.01, 0.02))
    torch.cuda.synchronize()
    assert torch.equal(gor, gow) and torch.equal(gsr, gsw)
    so = _sig(opa)
    np.testing.assert_allclose(gow.cpu().numpy(), go0 + 0.01 / n * so * (1 - so), rtol=1e-5, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. SSIM at 1920x1080 and at its edges
# ---------------------------------------------------------------------------------------------------------------------------
def ssim_terms_np(x, y):
    """fp64 SSIM restated over [..., H, W]: the SSIM map and the analytic gradient of its sum w.r.t. x,
    G*(dm/dmu1) + 2x G*(dm/dsigma1^2) + y G*(dm/dsigma12), with dm/dmu1 the total derivative through sigma1^2 and sigma12."""
    g = gauss_window()
    mu1, mu2 = conv_same(x, g), conv_same(y, g)
    s1 = conv_same(x * x, g) - mu1 * mu1
    s2 = conv_same(y * y, g) - mu2 * mu2
    s12 = conv_same(x * y, g) - mu1 * mu2
    A = mu1 * mu1 + mu2 * mu2 + SSIM_C1
    B = s1 + s2 + SSIM_C2
    Cn = 2 * mu1 * mu2 + SSIM_C1
    Dn = 2 * s12 + SSIM_C2
    m = Cn * Dn / (A * B)
    dm_ds1 = -m / B                                     # d/d sigma1^2
    dm_ds12 = 2 * Cn / (A * B)                          # d/d sigma12
    dm_dmu1 = 2 * mu2 * Dn / (A * B) - 2 * mu1 * m / A  # d/d mu1 with the sigmas held
    dm_dmu1 = dm_dmu1 - 2 * mu1 * dm_ds1 - mu2 * dm_ds12
    grad = conv_same(dm_dmu1, g) + 2 * x * conv_same(dm_ds1, g) + y * conv_same(dm_ds12, g)
    return m, grad


def _ssim_gpu(x, y, dev, w=None):
    """-> (mean SSIM, d mean SSIM / dx, and for w: the fused loss gradient and l1 sum) from the HIP kernels"""
    import torch
    from divshot_amd.train_ops import Ssim
    H, W = x.shape[1:]
    xd = torch.tensor(x, dtype=torch.float32, device=dev); yd = torch.tensor(y, dtype=torch.float32, device=dev)
    s = Ssim(W, H, dev)
    val = float(s.forward(xd, yd).item())
    g = s.backward(xd, yd, torch.full_like(xd, float("nan")), 1.0, accumulate=False).cpu().numpy()
    fused = None
    if w is not None:
        dL, l1 = s.loss_backward(xd, yd, w)
        fused = dL.cpu().numpy(), float(l1.item())
    return val, g, fused


def _region_worst(err, H, W):
    """worst error on the 16-pixel tile seams, within 5 pixels of the image border, and in the interior"""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    border = (yy < 5) | (xx < 5) | (yy >= H - 5) | (xx >= W - 5)
    seam = ((yy % 16 == 0) | (yy % 16 == 15) | (xx % 16 == 0) | (xx % 16 == 15)) & ~border
    interior = ~border & ~seam
    e = err.max(0)
    return {k: float(e[msk].max()) if msk.any() else 0.0 for k, msk in (("seam", seam), ("border", border), ("interior", interior))}


SSIM_GRAD_BAR = 1e-3          # element-wise, relative to the max |gradient| of the map


def test_ssim_full_hd_every_pixel(gpu_device):
    """1920x1080 (68x120 tiles, 4096 atomic slots): mean SSIM against fp64, the WHOLE gradient map of dvs_ssim_backward against the
    fp64 analytic backward (worst pixel reported per region: tile seams, border, interior), and dvs_loss_l1_ssim_backward + l1_sum
    likewise. Target quantised to k/255 (the plugin's 8-bit training views), render clipped to exact 0 / 1 in places."""
    rng = np.random.default_rng(1080)
    H, W, w = 1080, 1920, 0.2
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    base = 0.5 + 0.35 * np.sin(9 * xx + 5 * yy)[None] * np.array([1.0, 0.7, -0.8])[:, None, None]
    y = np.round(np.clip(base + 0.05 * rng.standard_normal((3, H, W)), 0, 1) * 255) / 255
    x = np.clip(y + 0.12 * rng.standard_normal((3, H, W)), 0, 1)
    x[:, 100:140, 200:260] = y[:, 100:140, 200:260]                 # exact ties: sign(0) = 0 in the L1 part
    x[:, 500:520] = 0.25                                             # a constant band
    x = x.astype(np.float32).astype(np.float64); y = y.astype(np.float32).astype(np.float64)
    assert (x == 0).any() and (x == 1).any()
    val, g, (dL, l1) = _ssim_gpu(x, y, gpu_device, w=w)
    m, grad = ssim_terms_np(x, y)
    N = x.size
    assert abs(val - m.mean()) < 1e-5, (val, m.mean())
    ref = grad / N
    err = np.abs(g - ref) / np.abs(ref).max()
    worst = _region_worst(err, H, W)
    print("ssim 1080p backward worst |err|/max:", worst)
    assert max(worst.values()) < SSIM_GRAD_BAR, worst
    ref_f = (1 - w) / N * np.sign(x - y) - w * ref
    err_f = np.abs(dL - ref_f) / (w * np.abs(ref).max())
    worst_f = _region_worst(err_f, H, W)
    print("fused l1+ssim backward worst |err|/max(ssim part):", worst_f)
    assert max(worst_f.values()) < SSIM_GRAD_BAR, worst_f
    want_l1 = (1 - w) * np.abs(x - y).mean()
    assert abs(l1 - want_l1) < 1e-5 * want_l1, (l1, want_l1)


def _fd_grad_mean_ssim(x, y, e=1e-5, batch=256):
    """fp64 central differences of the mean SSIM at every pixel, batched: one perturbed image per pixel"""
    P = x.size
    out = np.empty(P)
    for b0 in range(0, P, batch):
        k = min(batch, P - b0)
        E = np.zeros((k, P)); E[np.arange(k), b0 + np.arange(k)] = e
        E = E.reshape((k,) + x.shape)
        yb = np.broadcast_to(y, E.shape)
        mp, _ = ssim_terms_np(x[None] + E, yb)
        mm, _ = ssim_terms_np(x[None] - E, yb)
        out[b0:b0 + k] = (mp.reshape(k, -1).mean(1) - mm.reshape(k, -1).mean(1)) / (2 * e)
    return out.reshape(x.shape)


def _edge_inputs(H, W, rng):
    y = rng.uniform(0, 1, (3, H, W))
    yield "random", np.clip(y + 0.15 * rng.standard_normal((3, H, W)), 0, 1), y
    yield "constant", np.full((3, H, W), 0.3), np.full((3, H, W), 0.6)
    sat_x = (rng.random((3, H, W)) < 0.5).astype(np.float64)
    yield "saturated", sat_x, np.where(rng.random((3, H, W)) < 0.3, sat_x, 1 - sat_x)
    yield "quantised", np.clip(y + 0.1 * rng.standard_normal((3, H, W)), 0, 1), np.round(y * 255) / 255


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (5, 3), (11, 10), (10, 11), (16, 16), (16, 17), (17, 16), (21, 32)])
def test_ssim_edge_shapes(gpu_device, H, W):
    """Images smaller than one tile and than the 11-tap window, one tile exactly, one pixel over a tile, a width of whole tiles over a
    ragged height; random, constant (zero variance: C1 / C2 decide), 0/1-saturated and 8-bit-quantised inputs. Mean SSIM against fp64,
    the gradient at EVERY pixel against the fp64 analytic backward and against fp64 central differences."""
    rng = np.random.default_rng(H * 100 + W)
    for kind, x, y in _edge_inputs(H, W, rng):
        x = x.astype(np.float32).astype(np.float64); y = y.astype(np.float32).astype(np.float64)
        val, g, (dL, l1) = _ssim_gpu(x, y, gpu_device, w=0.2)
        m, grad = ssim_terms_np(x, y)
        N = x.size
        assert abs(val - m.mean()) < 2e-5, (kind, val, m.mean())
        ref = grad / N
        fd = _fd_grad_mean_ssim(x, y)
        scale = max(np.abs(ref).max(), 1e-3 / N)                   # (x, y constant and equal would have a zero gradient)
        assert np.abs(ref - fd).max() <= 1e-6 * scale + 1e-9, (kind, "restatement vs central differences")
        err = np.abs(g - ref).max() / scale
        assert err < SSIM_GRAD_BAR, (kind, err)
        ref_f = 0.8 / N * np.sign(x - y) - 0.2 * ref
        assert np.abs(dL - ref_f).max() < SSIM_GRAD_BAR * 0.2 * scale + 1e-6 * 0.8 / N, kind
        assert abs(l1 - 0.8 * np.abs(x - y).mean()) <= 1e-6 * max(np.abs(x - y).mean(), 1e-3), kind


# ---------------------------------------------------------------------------------------------------------------------------
# 6. Adam at product scale
# ---------------------------------------------------------------------------------------------------------------------------
def test_adam_groups_at_scale_visible_and_active_chunks(gpu_device):
    """dvs_adam_step_groups at 1 000 003 splats with the plugin's six groups in one launch, shN tiled with its last tile padded,
    active_chunks at SH degree 1 AND a per-step `visible` mask, three steps against the fp64 textbook recurrences. Padding lanes,
    inactive chunks and invisible splats stay bit-identical."""
    import torch
    from divshot_amd.train_ops import adam_step_groups
    from divshot_amd.raster import shn_rows_to_tiled_np, shn_tiled_to_rows_np
    n = 1_000_003
    assert n % 64 == 3
    rng = np.random.default_rng(6)
    widths = {"pos": 3, "sh0": 3, "shN": 45, "opacity": 1, "scale": 3, "rot": 4}
    lrs = {"pos": 1.6e-4, "sh0": 2.5e-3, "shN": 1.25e-4, "opacity": 5e-2, "scale": 5e-3, "rot": 1e-3}
    b1, b2, eps = 0.9, 0.999, 1e-15
    b1_32, b2_32 = float(np.float32(b1)), float(np.float32(b2))    # what the kernel receives (1 - b2 is then 1.3e-5 off 1e-3)
    active = 3                                                      # degree 1: 9 coefficients -> ceil(9/4) float4 chunks
    H = {}
    for k, w in widths.items():
        p = rng.standard_normal((n, w)).astype(np.float32)
        mv = [np.abs(rng.standard_normal((n, w))).astype(np.float32) * s for s in (1e-2, 1e-4)]
        if k == "shN":
            for a in mv:
                a[:, 9:] = 0                                        # above degree 1: no gradient ever, zero moments
        H[k] = [p] + mv
    vis_steps = [((rng.random(n) < p_) * rng.integers(1, 60, n)).astype(np.int32) for p_ in (0.7, 0.5, 0.9)]
    grads = []
    for _ in range(3):
        gk = {k: rng.standard_normal((n, w)).astype(np.float32) * 0.01 for k, w in widths.items()}
        gk["shN"][:, 9:] = 0
        grads.append(gk)

    def dev_arr(k, a, pad_value):
        if k != "shN":
            return torch.tensor(a.reshape(-1), device=gpu_device)
        t = shn_rows_to_tiled_np(a).reshape(-1, 12, 64, 4)
        t[-1, :, n % 64:, :] = pad_value                            # padding lanes of the last tile
        return torch.tensor(t.reshape(-1), device=gpu_device)

    D = {k: [dev_arr(k, a, v) for a, v in zip(H[k], (7.0, 3.0, 5.0))] for k in widths}
    shn_start = [x.clone() for x in D["shN"]]
    for t_, (gk, vis) in enumerate(zip(grads, vis_steps), start=1):
        gd = {k: dev_arr(k, gk[k], 1.0) for k in widths}
        groups = [dict(param=D[k][0], grad=gd[k], m=D[k][1], v=D[k][2], lr=lrs[k], width=w, tiled=(k == "shN"),
                       active_chunks=(active if k == "shN" else 0)) for k, w in widths.items()]
        adam_step_groups(groups, t_, beta1=b1, beta2=b2, eps=eps, visible=torch.tensor(vis, device=gpu_device))
    torch.cuda.synchronize()
    for k, w in widths.items():
        cols = slice(0, 4 * active) if k == "shN" else slice(0, w)  # the floats the kernel may touch
        p, m, v = (a[:, cols].astype(np.float64) for a in H[k])
        for t_, (gk, vis) in enumerate(zip(grads, vis_steps), start=1):
            on = (vis > 0)[:, None]
            if k == "shN":
                g = np.zeros((n, 4 * active)); g[:, :9] = gk[k][:, :9]
            else:
                g = gk[k].astype(np.float64)
            m2 = b1_32 * m + (1 - b1_32) * g; v2 = b2_32 * v + (1 - b2_32) * g * g
            p2 = p - lrs[k] * (m2 / (1 - b1_32 ** t_)) / (np.sqrt(v2 / (1 - b2_32 ** t_)) + eps)
            p, m, v = np.where(on, p2, p), np.where(on, m2, m), np.where(on, v2, v)
        got = [x.cpu().numpy() for x in D[k]]
        if k == "shN":
            rows = [shn_tiled_to_rows_np(a, n).reshape(n, 45) for a in got]
            for a, b in zip(got, shn_start):                        # padding lanes and the chunks above the active ones: untouched
                a4, b4 = a.reshape(-1, 12, 64, 4), b.cpu().numpy().reshape(-1, 12, 64, 4)
                assert np.array_equal(a4[-1, :, n % 64:], b4[-1, :, n % 64:]) and np.array_equal(a4[:, active:], b4[:, active:])
            got = [r[:, cols] for r in rows]
        else:
            got = [a.reshape(n, w) for a in got]
        never = ~np.any([vis > 0 for vis in vis_steps], 0)
        assert never.any()
        for j, (a, r, start) in enumerate(zip(got, (p, m, v), H[k])):
            assert np.array_equal(a[never], start[never][:, cols]), (k, j)
            # m: a few ulp of |g| ~ 1e-2 where the update cancels; p: that error through lr / sqrt(v) (the 1e-6 bar of test_l1_and_adam at lr 1e-2)
            tol = ((2e-5, 1e-4 * lrs[k]), (1e-5, 1e-8), (1e-5, 1e-12))[j]
            np.testing.assert_allclose(a, r, rtol=tol[0], atol=tol[1], err_msg=f"{k} {'pmv'[j]}")
