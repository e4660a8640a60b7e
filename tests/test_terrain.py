"""Terrain generator (row f-4): bit-exact against height samples minted from the reference's own Terrain class
(tests/golden/terrain_ref.npz, oracle/make_terrain_goldens.py), live against the reference where it is present, and
the specification of the one tile type whose reference code no longer runs (scipy's interp2d was removed)."""
import os, sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from isaacgymdyros_amd.terrain import Terrain, TerrainCfg, Tile, random_uniform, _bilinear_resample
from oracle.make_terrain_goldens import CASES

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "terrain_ref.npz"))


@pytest.mark.parametrize("name,seed,ov", CASES, ids=[c[0] for c in CASES])
def test_matches_reference_samples(name, seed, ov):
    t = Terrain(TerrainCfg(**ov), 64, seed=seed)
    ref_h, ref_o = GOLD[name + "/heightsamples"], GOLD[name + "/env_origins"]
    assert t.heightsamples.dtype == np.int16 and t.heightsamples.shape == ref_h.shape
    assert np.array_equal(t.heightsamples, ref_h)
    assert np.array_equal(t.env_origins, ref_o)
    assert (t.tot_rows, t.tot_cols) == ref_h.shape
    if ov["mesh_type"] == "trimesh":          # triangle mesh with straightened steep faces: digests of the reference's arrays
        import hashlib
        assert tuple(GOLD[name + "/vertices_shape"]) == t.vertices.shape and str(GOLD[name + "/vertices_dtype"]) == str(t.vertices.dtype)
        assert tuple(GOLD[name + "/triangles_shape"]) == t.triangles.shape and str(GOLD[name + "/triangles_dtype"]) == str(t.triangles.dtype)
        for arr, key in ((t.vertices, "vertices"), (t.triangles, "triangles")):
            dg = np.frombuffer(hashlib.sha256(np.ascontiguousarray(arr).tobytes()).digest(), dtype=np.uint8)
            assert np.array_equal(dg, GOLD[name + "/" + key + "_sha256"]), key


def test_live_against_reference_when_present():
    """Live against the reference's Terrain where it is mounted; everywhere against its samples recorded in
    tests/golden/reference_live.npz (oracle/make_live_goldens.py)."""
    import reference_cases as RC
    from oracle import ref_harness
    g = np.load(os.path.join(ROOT, "tests", "golden", "reference_live.npz"))
    for seed in RC.TERRAIN_SEEDS:
        m = Terrain(TerrainCfg(**RC.TERRAIN_LIVE), 8, seed=seed)
        refs = [(g["terrain/%d/heightsamples" % seed], g["terrain/%d/env_origins" % seed])]
        if ref_harness.available():
            refs.append(RC.reference_terrain(seed))
        for h, o in refs:
            assert np.array_equal(m.heightsamples, h) and np.array_equal(m.env_origins, o)


def test_plane_builds_nothing():
    t = Terrain(TerrainCfg(), 16)
    assert not hasattr(t, "heightsamples")


def test_rough_slope_specification():
    # coarse grid every 0.2 m, bilinear in between, rounded to samples: nodes of the coarse grid are reproduced and
    # every sample lies inside the range drawn
    rs = np.random.RandomState(4)
    coarse = rs.choice(np.arange(-10, 11), (5, 7))
    up = _bilinear_resample(coarse, 9, 13)
    assert np.allclose(up[::2, ::2], coarse)
    assert np.allclose(up[1, 0], 0.5 * (coarse[0, 0] + coarse[1, 0]))
    t = Tile(80, 80, 0.005, 0.1)
    random_uniform(t, np.random.RandomState(1), -0.05, 0.05, step=0.005, downsampled_scale=0.2)
    assert t.height_field_raw.min() >= -10 and t.height_field_raw.max() <= 10 and t.height_field_raw.std() > 1
    full = Terrain(TerrainCfg(mesh_type="heightfield", curriculum=True, num_rows=2, num_cols=10, border_size=1), 4, seed=0)
    assert full.heightsamples.shape == (2 * 80 + 20, 10 * 80 + 20)


@pytest.mark.parametrize("args", [dict(min_height=-0.05, max_height=0.05, step=0.005, downsampled_scale=0.2),    # utils/terrain.py:128-130 (curriculum)
                                  dict(min_height=-0.1, max_height=0.1, step=0.025, downsampled_scale=0.2),     # tasks/amp/tocabi_amp_lower_base.py:1204
                                  dict(min_height=-0.1, max_height=0.1, step=0.05, downsampled_scale=0.2)])    # :1151
def test_random_uniform_against_scipys_replacement_of_interp2d(args):
    """`random_uniform_terrain` (python/isaacgym/terrain_utils.py:17-51) cannot run on this image: it calls
    `scipy.interpolate.interp2d`, removed in SciPy 1.14, whose removal notice names `RectBivariateSpline` as the "nearly
    bug-for-bug compatible" replacement on regular grids.  This restates the reference's lines with that one substitution --
    same draws (`choice` over `arange(min, max + step, step)`), same argument order f(y, x) with z of shape (len(x), len(y)), same
    `linspace` nodes, `np.rint`, int16 accumulation -- and holds the package's generator to it sample for sample, for the
    arguments of all three call sites in the reference."""
    from scipy.interpolate import RectBivariateSpline
    for seed in range(6):
        t = Tile(80, 80, 0.005, 0.1)
        t.height_field_raw += np.random.RandomState(100 + seed).randint(-3, 4, size=(80, 80)).astype(np.int16)      # (accumulates onto a slope)
        base = t.height_field_raw.copy()
        random_uniform(t, np.random.RandomState(seed), **args)
        # the reference's body
        rs = np.random.RandomState(seed)
        lo, hi, st = int(args["min_height"] / 0.005), int(args["max_height"] / 0.005), int(args["step"] / 0.005)
        heights_range = np.arange(lo, hi + st, st)
        coarse = rs.choice(heights_range, (int(80 * 0.1 / args["downsampled_scale"]), int(80 * 0.1 / args["downsampled_scale"])))
        x = np.linspace(0, 80 * 0.1, coarse.shape[0])
        y = np.linspace(0, 80 * 0.1, coarse.shape[1])
        f = RectBivariateSpline(y, x, coarse.T.astype(np.float64), kx=1, ky=1, s=0)        # interp2d(y, x, z, kind='linear')
        xu, yu = np.linspace(0, 80 * 0.1, 80), np.linspace(0, 80 * 0.1, 80)
        z = np.rint(f(yu, xu).T)                                                              # f(y_upsampled, x_upsampled): rows = x
        assert np.array_equal(t.height_field_raw, base + z.astype(np.int16)), seed
        assert np.abs(z).max() > 0


def test_height_lookup_is_bilinear():
    t = Terrain(TerrainCfg(mesh_type="heightfield", curriculum=True, num_rows=2, num_cols=2, border_size=1,
                           terrain_proportions=[1.0, 0.0, 0.0, 0.0, 0.0]), 4, seed=0)
    c = t.cfg
    i, j = 37, 52
    x, y = i * c.horizontal_scale - c.border_size, j * c.horizontal_scale - c.border_size
    assert np.isclose(t.height_at(x, y), t.heightsamples[i, j] * c.vertical_scale)
    mid = t.height_at(x + 0.5 * c.horizontal_scale, y)
    assert np.isclose(mid, 0.5 * (t.heightsamples[i, j] + t.heightsamples[i + 1, j]) * c.vertical_scale)
