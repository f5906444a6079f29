"""dvs_lod_merge_count / dvs_lod_merge_write against tests/lod_ref.py at the smallest shapes where each part can go wrong: n = 0 and 1,
the wavefront edge (64, 65), DVS_SCAN_TILE + 1 = 2049, 300 splats in one cell (a long serial walk), every splat alone in its cell
(the output is the input, bit for bit, in key order), non-finite splats with weightless clusters, and a cluster of thin, nearly
coplanar splats (sigma ratio 1e3: the eigenvalue floor and the two-pass moment); SH degree 0 and 3, both shN layouts in and out.

Exact: m, n_dropped, the order of the clusters, the rows of single-member clusters, the zero bands above D, the tiled pads.
Toleranced, against the float64 restatement: mu, the SH rows, alpha', and for the geometry the reconstructed R diag(e^{2 s}) R^T as a
relative Frobenius distance (raw scale and rot are never compared: the eigenbasis is ambiguous under sign, order and repeated
eigenvalues).

The bounds. The float32 restatement (numpy, the device's operation order) was run against the float64 one on the CPU over exactly the
cases below (both degrees); MEASURED_* are its worst errors, and the device is allowed 4 x that: its exp, log and division differ from
numpy's by a few ulp and nothing else does. Units: mu relative to the largest coordinate of the finite centres (a mean's rounding
error scales with the size of the coordinates, not with the cell); SH absolute (the rows are O(1)); alpha' absolute; geometry relative
Frobenius."""
import functools
import numpy as np
import pytest
import lod_ref as L

pytestmark = pytest.mark.gpu

# worst over the cases (mu at mix, the others at n2049 with its 461 merged clusters; the 300-member and the thin cluster stay below them)
MEASURED_MU, MEASURED_SH, MEASURED_ALPHA, MEASURED_COV = 2.148e-07, 6.383e-07, 7.768e-07, 6.878e-07
BOUND_MU, BOUND_SH, BOUND_ALPHA, BOUND_COV = 4 * MEASURED_MU, 4 * MEASURED_SH, 4 * MEASURED_ALPHA, 4 * MEASURED_COV


def random_splats(n, seed, lo=-1.0, hi=1.0):
    r = np.random.default_rng(seed)
    return {"pos": r.uniform(lo, hi, (n, 3)).astype(np.float32), "sh0": r.normal(0, 0.5, (n, 3)).astype(np.float32),
            "shN": r.normal(0, 0.2, (n, 45)).astype(np.float32), "opacity": r.normal(0, 2, n).astype(np.float32),
            "scale": r.normal(-3.0, 0.5, (n, 3)).astype(np.float32), "rot": r.normal(0, 1, (n, 4)).astype(np.float32)}


def lattice(lo, hi, res):
    o, c, d = L.lattice_for([lo] * 3 + [hi] * 3, res)
    return o, c, d


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (params, (origin, cell, dims))"""
    if name.startswith("n"):                                                # n1, n64, n65, n2049: about four members per cell
        n = int(name[1:])
        res = {1: 4, 64: 4, 65: 4, 2049: 8}[n]
        return random_splats(n, n), lattice(-1.0, 1.0, res)
    if name == "one_cell":                                                   # 300 splats in the cell (1, 2, 3) of 4^3
        p = random_splats(300, 7)
        p["pos"] = (p["pos"] * np.float32(0.2) + np.array([-0.25, 0.25, 0.75], np.float32)).astype(np.float32)
        return p, lattice(-1.0, 1.0, 4)
    if name == "alone":                                                      # 6^3 = 216 cells, one splat each, in shuffled order
        p = random_splats(216, 8)
        g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(216, 3)
        p["pos"] = ((g[np.random.default_rng(9).permutation(216)] + 0.5) / 3.0 - 1.0).astype(np.float32)
        return p, lattice(-1.0, 1.0, 6)
    if name == "mix":
        p = random_splats(700, 10)
        p["pos"][5, 0] = np.nan; p["pos"][70, 2] = np.inf; p["pos"][133, 1] = -np.inf; p["scale"][200, 1] = np.nan; p["rot"][201, 3] = np.inf
        o, c, d = lattice(-1.0, 1.0, 4)
        keys = L.cell_keys(p["pos"], o, c, d)
        p["opacity"][keys == 21] = -np.inf                                   # a cluster whose members are all dropped: the cell vanishes
        p["scale"][keys == 42] = -1000.0                                     # W = 0: sigma underflows to 0 in every precision
        p["scale"][keys == 63] = -1000.0
        p["opacity"][np.nonzero(keys == 7)[0][::2]] = -np.inf                # a cluster that loses every other member
        lone = np.nonzero(keys == 11)[0]
        p["pos"][lone[1:], 0] = np.nan                                       # one survivor, weightless: a single member is copied whatever its weight
        p["scale"][lone[0]] = -1000.0
        return p, (o, c, d)
    if name == "thin":                                                       # 40 nearly coplanar discs (sigma 3e-2, 3e-2, 3e-5) in one cell
        r = np.random.default_rng(11)
        p = random_splats(40, 12)
        u, v = np.array([1.0, 0.3, -0.2]), np.array([0.1, 1.0, 0.4])
        nrm = np.cross(u, v); nrm /= np.linalg.norm(nrm)
        u /= np.linalg.norm(u); v = np.cross(nrm, u)
        ab = r.uniform(-0.2, 0.2, (40, 2))
        p["pos"] = (np.array([0.25, 0.25, 0.25]) + ab[:, :1] * u + ab[:, 1:] * v + r.normal(0, 1e-6, (40, 1)) * nrm).astype(np.float32)
        p["scale"] = (np.log([3e-2, 3e-2, 3e-5]) + r.normal(0, 0.05, (40, 3))).astype(np.float32)
        R = np.stack([u, v, nrm], 1)                                         # columns: the discs' axes
        q0 = L.quat_of_rotation(R, np.float64)
        p["rot"] = ((q0 + r.normal(0, 1e-5, (40, 4))) * r.uniform(0.5, 2.0, (40, 1))).astype(np.float32)
        return p, lattice(-1.0, 1.0, 4)
    raise KeyError(name)


CASES = ("n1", "n64", "n65", "n2049", "one_cell", "alone", "mix", "thin")


@functools.lru_cache(maxsize=None)
def reference(name, D, dtype=np.float64):
    p, (o, c, d) = case(name)
    return L.merge(p, o, c, d, D, dtype)


def extent(pos):
    """the largest |coordinate| over the centres whose three coordinates are finite"""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    return float(np.abs(pos[np.isfinite(pos).all(1)]).max())


def errors(got, ref, info, size):
    """the four toleranced quantities of `got` (float32 rows) against the float64 restatement, over the multi-member clusters; size =
    extent() of the input"""
    multi = ~info["single"]
    if not multi.any():
        return 0.0, 0.0, 0.0, 0.0
    g = {k: np.asarray(v, np.float64)[multi] for k, v in got.items()}
    r = {k: v[multi] for k, v in ref.items()}
    e_mu = np.abs(g["pos"] - r["pos"]).max() / size
    e_sh = max(np.abs(g["sh0"] - r["sh0"]).max(), np.abs(g["shN"] - r["shN"]).max())
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    e_alpha = np.abs(sig(g["opacity"]) - sig(r["opacity"])).max()
    a, b = L.written_covariances(g["scale"], g["rot"]), L.written_covariances(r["scale"], r["rot"])
    fro = lambda c6: np.sqrt((c6 ** 2 * np.array([1, 2, 2, 1, 2, 1])).sum(1))
    e_cov = (fro(a - b) / fro(b)).max()
    return e_mu, e_sh, e_alpha, e_cov


def run(dev, name, D, lin, lout):
    import torch
    from divshot_amd import lod as LOD
    from divshot_amd.raster import shn_rows_to_tiled_np, shn_tiled_to_rows_np
    p, (o, c, d) = case(name)
    n = len(p["opacity"])
    t = {k: torch.from_numpy(v).to(dev) for k, v in p.items()}
    if lin == 1:
        t["shN"] = torch.from_numpy(shn_rows_to_tiled_np(p["shN"])).to(dev)
    # NaN everywhere the kernels do not write: room for n rows
    room = {k: torch.full((max(n, 1) * w,), float("nan"), device=dev) for k, w in (("pos", 3), ("sh0", 3), ("opacity", 1), ("scale", 3), ("rot", 4))}
    room["shN"] = torch.full((((max(n, 1) + 63) // 64) * 64 * 48 if lout == 1 else max(n, 1) * 45,), float("nan"), device=dev)
    out, counts = LOD.merge_splats(t, lattice=LOD.make_lattice(o, c, d), sh_degree=D, shn_layout=lin, shn_layout_out=lout, n=n, out=room)
    m = counts["m"]
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert all(torch.isnan(room[k].reshape(-1)[out[k].numel():]).all() for k in L.KEYS), "nothing is written past the m rows"
    if lout == 1:
        flat = got["shN"]
        assert flat.size == ((m + 63) // 64) * 64 * 48
        tiles = flat.reshape(-1, 12, 64, 4)
        assert (tiles[:, 11, :, 1:] == 0).all(), "the three pad floats of a tiled output are 0"
        lanes = np.arange(tiles.shape[0] * 64).reshape(-1, 64)
        assert (tiles.transpose(0, 2, 1, 3)[lanes >= m] == 0).all(), "the lanes past m are 0"
        got["shN"] = shn_tiled_to_rows_np(flat, m).reshape(m, 45) if m else np.zeros((0, 45), np.float32)
    return got, counts


def check(dev, name, D, lin, lout):
    ref, info = reference(name, D)
    got, counts = run(dev, name, D, lin, lout)
    assert counts == {"m": info["m"], "n_dropped": info["n_dropped"]}, (counts, info["m"], info["n_dropped"])
    p, (o, c, d) = case(name)
    single = info["single"]
    for k in L.KEYS:                                                         # single members, bit for bit: this also pins the clusters' order
        want = ref[k][single].astype(np.float32)
        assert np.array_equal(got[k][single].view(np.uint32), want.view(np.uint32)), (name, k)
    assert np.array_equal(L.cell_keys(got["pos"], o, c, d), info["keys"]), "clusters in ascending cell key, each mean inside its cell"
    assert (got["shN"][~single][:, L.LIMIT[D]:] == 0).all(), "the bands above D are written as 0"
    assert np.isfinite(np.concatenate([got[k][~single].reshape(-1) for k in L.KEYS])).all()
    q = got["rot"][~single].astype(np.float64)
    assert (np.abs(np.linalg.norm(q, axis=1) - 1.0) <= 1e-6).all() and (q[:, 0] >= 0).all()
    e = errors(got, ref, info, extent(p["pos"]))
    print(f"{name} D={D} in={lin} out={lout}: n={len(p['opacity'])} m={counts['m']} dropped={counts['n_dropped']} multi={int((~single).sum())} "
          f"mu {e[0]:.3e} (<= {BOUND_MU:.3e}) sh {e[1]:.3e} (<= {BOUND_SH:.3e}) alpha {e[2]:.3e} (<= {BOUND_ALPHA:.3e}) cov {e[3]:.3e} (<= {BOUND_COV:.3e})")
    assert e[0] <= BOUND_MU and e[1] <= BOUND_SH and e[2] <= BOUND_ALPHA and e[3] <= BOUND_COV, e


def test_no_splats(gpu_device):
    import torch
    from divshot_amd import lod as LOD
    t = {k: torch.zeros((4, w) if w else (4,), device=gpu_device) for k, w in (("pos", 3), ("sh0", 3), ("shN", 45), ("opacity", 0), ("scale", 3), ("rot", 4))}
    out, counts = LOD.merge_splats(t, lattice=LOD.make_lattice([0, 0, 0], 1.0, [4, 4, 4]), n=0)
    assert counts == {"m": 0, "n_dropped": 0} and out["pos"].shape[0] == 0


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("D,lin,lout", [(3, 0, 0), (0, 1, 1)])
def test_merge_matches_the_restatement(gpu_device, name, D, lin, lout):
    check(gpu_device, name, D, lin, lout)


@pytest.mark.parametrize("lin,lout", [(0, 1), (1, 0)])
def test_layouts_cross(gpu_device, lin, lout):
    check(gpu_device, "n65", 3, lin, lout)
    check(gpu_device, "mix", 3, lin, lout)


def test_every_splat_alone_is_the_input_in_key_order(gpu_device):
    p, (o, c, d) = case("alone")
    got, counts = run(gpu_device, "alone", 0, 0, 1)                          # (degree 0: a single member still keeps every band)
    order = np.argsort(L.cell_keys(p["pos"], o, c, d), kind="stable")
    assert counts == {"m": 216, "n_dropped": 0}
    for k in L.KEYS:
        assert np.array_equal(got[k].view(np.uint32), p[k][order].view(np.uint32)), k


def test_two_runs_return_identical_bytes(gpu_device):
    a, ca = run(gpu_device, "n2049", 3, 0, 0)
    b, cb = run(gpu_device, "n2049", 3, 0, 0)
    assert ca == cb and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in L.KEYS)
