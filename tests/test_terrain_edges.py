"""The height-field instantiation of the step kernels at the edges of the map, of the sample grid and of the coarse bound table, on the
CPU: the scenes of tests/terrain_edge_cases.py through the host emulation of the kernel source against the oracle; the bound table
(dw_physics.h terrain_bound_cell / terrain_bound, which has no export) restated in numpy and held to the invariant that makes it safe,
on the oracle's data; and the conditions under which those checks mean something -- every scene reaches the edge it is named for, and
the pillar scene breaks the invariant as soon as the table is built wrongly (tests/test_terrain_edges_gpu.py runs the same scenes on
the MI355X)."""
import numpy as np
import pytest

import terrain_edge_cases as TE
from emul_backend import EmulSim
from isaacgymdyros_amd.terrain import Terrain, TerrainCfg
from oracle.oracle import OracleSim

BITE_PAIRS = 8          # loaded (env, body) pairs a wrong table must drop, per way of being wrong: a condition on the scene


def test_fk_agrees_with_the_oracle():
    """The numpy chain that places the scenes' contact points, against the oracle's body-position entry point (double precision)."""
    rng = np.random.default_rng(1)
    N = 32
    sim = OracleSim(N)
    sim.buf["root_states"][:, :3] = rng.normal(size=(N, 3))
    q = rng.normal(size=(N, 4))
    sim.buf["root_states"][:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    sim.buf["dof_state"][..., 0] = rng.uniform(-1.2, 1.2, size=(N, 33))
    x, _ = TE.fk(sim.buf["root_states"], sim.buf["dof_state"][..., 0])
    assert np.abs(x - TE.oracle_body_origins(sim)).max() < 2e-6
    assert abs(TE.model_reach() - 1.476) < 1e-3          # (the robot's reach the window is sized by)


@pytest.mark.parametrize("wave_build", [1, 2, 3], ids=["keep", "two_waves", "hex"])
@pytest.mark.parametrize("name", list(TE.SCENES))
def test_edge_scene_vs_oracle_in_emulation(name, wave_build):
    """One substep of every scene through the kernel source (host emulation, each build) at the tolerances of
    tests/terrain_edge_cases.py."""
    got = TE.run_scene(lambda N, terrain: EmulSim(N, terrain=terrain, terrain_curriculum=0, debug_wave_build=wave_build), name)
    TE.check(name, got, label="emul wb%d" % wave_build)


def _generated(kind):
    """The two generated-terrain scenes of tests/test_terrain_physics.py (walking range; fallen on the highest tiles) as (field, root
    states, joint state), the map wrapped as a TE.Field."""
    walking = kind == "walking"
    t = (Terrain(TerrainCfg(mesh_type="heightfield", curriculum=True, num_rows=2, num_cols=4, border_size=2, terrain_proportions=[0.2, 0.2, 0.3, 0.3, 0.0]), 8, seed=3)
         if walking else
         Terrain(TerrainCfg(mesh_type="heightfield", curriculum=True, num_rows=3, num_cols=5, border_size=2, terrain_proportions=[0.1, 0.2, 0.35, 0.25, 0.1]), 15, seed=11))
    field = TE.Field(t.heightsamples, t.cfg.horizontal_scale, t.cfg.vertical_scale, t.cfg.border_size)
    rng = np.random.default_rng(5 if walking else 2)
    N = 64
    org = t.env_origins.reshape(-1, 3)
    if not walking:
        org = org[np.argsort(-org[:, 2])][:8]
    xy = org[rng.integers(0, len(org), size=N), 0:2] + rng.uniform(-3.5, 3.5, size=(N, 2))
    if walking:
        root, dof = np.zeros((N, 13), np.float32), np.zeros((N, 33, 2), np.float32)
        root[:, 0:2], root[:, 6] = xy, 1.0
        root[:, 2] = field.height_at(xy[:, 0], xy[:, 1]) + 0.93 + rng.uniform(-0.03, 0.05, size=N)
        dof[:, :, 0] = TE.Q0 + rng.normal(size=(N, 33)) * 0.05
    else:
        root, dof = TE._fallen(field, xy, rng)
    return field, root, dof


def _table_data(name):
    """(field, root states, body origins, the pairs the ground loads) of a scene, all from the oracle."""
    if name.startswith("generated_"):
        field, root, dof = _generated(name[len("generated_"):])
        sim = OracleSim(len(root), terrain=field, terrain_curriculum=0, self_collision=0)
        sim.buf["root_states"][...], sim.buf["dof_state"][...] = root, dof
        origins = TE.oracle_body_origins(sim)
        sim.simulate(np.zeros((len(root), 33), np.float32))
        return field, root, origins, TE.loaded_pairs(sim.buf["contact_forces"])
    field, root, _, _ = TE.scene(name)
    return field, root, TE.initial_origins(name), TE.loaded_pairs(TE.ground_forces(name))


@pytest.mark.parametrize("name", list(TE.SCENES) + ["generated_walking", "generated_fallen"])
def test_bound_table_invariant_on_the_oracles_data(name):
    """With the real cell and reach window, no body that the oracle's ground contact loads has its origin higher above the bound of its
    robot's cell than its bounding radius: skipping on that test loses nothing.  (The radius is offset + extent per primitive; the
    kernels add 1 % and 1 mm to it.)"""
    field, root, origins, pairs = _table_data(name)
    cell, reach = TE.cell_samples(field.hscale), TE.reach_samples(field.hscale)
    table = TE.bound_table(field.heightsamples, cell, reach)
    assert table.shape == (-(-field.tot_rows // cell), -(-field.tot_cols // cell))
    above = TE.above_bound(field, root, origins, pairs, table, cell)
    print("%-20s cell %d reach %d table %s: %d loaded pairs, nearest to the bound %.3f m" % (name, cell, reach, table.shape, len(above), above.max(initial=-np.inf)))
    assert (above <= 0).all(), (name, float(above.max()))
    if name in ("walls", "fallen_at_the_edge", "generated_fallen"):
        assert len(above) >= 200, len(above)          # (bodies other than the feet are on the ground, many of them)


def test_cell_and_reach_at_the_scales_of_the_scenes():
    """hm_cell_samples / hm_reach_samples restated: 0.1 -> 5 and 16, 0.07 -> 7 and 23, 0.25 -> 2 and 7, 0.5 -> 1 and 4, 1.0 -> (int)0.5
    = 0 floored to 1, and 3; the maps of the scale scenes end in a partial row and column of cells."""
    assert [TE.cell_samples(h) for h in (0.1, 0.07, 0.25, 0.5, 1.0)] == [5, 7, 2, 1, 1]
    assert [TE.reach_samples(h) for h in (0.1, 0.07, 0.25, 0.5, 1.0)] == [16, 23, 7, 4, 3]
    for name, (hscale, _, rows, cols) in TE.SCALES.items():
        cell = TE.cell_samples(hscale)
        assert rows != cols and (cell == 1 or (rows % cell and cols % cell)), name


def test_pillars_bite_on_the_reach_window():
    """A4 depends on the part of the table that looks into neighbouring cells: with no reach window (own cell only), with the window
    not widened on one side (+x, -x, +y, -y in turn) and with rows taken for cols (the map is 120 x 90), at least 8 loaded (env, body)
    pairs per case have their origin more than the radius above the wrong bound -- contacts a kernel with that table would drop, and
    the loaded-bodies check of the scene would report.

    A1 cannot be made to bite this way: its robots stand, only the soles are loaded, and the sole corners are sampled whatever the
    table says.  A5 (fallen robots on A1's field) loads ~900 pairs but its ground is +-40 mm with a 0.3 m ridge: a body on it is
    within its radius of almost any bound.  The non-square A4 carries the rows / cols case."""
    field, root, origins, pairs = _table_data("walls")
    cell, reach = TE.cell_samples(field.hscale), TE.reach_samples(field.hscale)
    dropped = lambda table, swap=False: int((TE.above_bound(field, root, origins, pairs, table, cell, swap=swap) > 0).sum())
    counts = {"reach 0": dropped(TE.bound_table(field.heightsamples, cell, 0))}
    for cut in ("+x", "-x", "+y", "-y"):
        counts["cut " + cut] = dropped(TE.bound_table(field.heightsamples, cell, reach, cut=cut))
    counts["rows for cols"] = dropped(TE.swapped_table(field, cell, reach), swap=True)
    print("walls: pairs a wrong table drops, of %d loaded:" % len(pairs[0]), counts)
    assert all(v >= BITE_PAIRS for v in counts.values()), counts
    # the touched pillar is 0.3 .. 0.9 m from the base, and the arms carry the loads
    e, mv, _ = pairs
    assert np.isin(mv, TE.ARM_BODIES + (20, 22, 30, 32)).sum() >= 100


def test_scenes_reach_what_they_are_named_for():
    """Counted in numpy from each scene's state, in the kernels' index arithmetic, so that a re-seeded scene cannot silently stop
    testing its edge: contact points and bases beyond each of the four edges of the map (the `u < 0` and `u > umax` clamps), in the
    last sample interval, with an exactly integral grid coordinate, and the cells of the bound table the bases index."""
    for name in ("borders", "borders_no_border", "fallen_at_the_edge"):
        r = TE.reach_counts(name)
        for tag, least in (("corners", 50), ("points", 300), ("bases", 8)):
            assert min(r[tag][k] for k in ("below_u", "above_u", "below_v", "above_v")) >= least, (name, tag, r[tag])
        assert r["corners"]["last_cell_u"] >= 10 and r["corners"]["last_cell_v"] >= 10, (name, r["corners"])
    r = TE.reach_counts("borders")
    assert r["bases"]["integral_u"] >= 20 and r["bases"]["integral_v"] >= 20, r["bases"]          # (sample 0 and the last sample line)
    hr, hc = r["table"]
    assert {ci for ci, _ in r["cells"]} >= {0, hr - 1} and {cj for _, cj in r["cells"]} >= {0, hc - 1}

    r = TE.reach_counts("lines")
    field, root, _, _ = TE.scene("lines")
    assert r["bases"]["integral_u"] >= 10 and r["bases"]["integral_v"] >= 10, r["bases"]          # bases exactly on a sample line
    assert r["corners"]["near_u"] >= 60 and r["corners"]["near_v"] >= 60, r["corners"]            # sole corners within 2e-5 samples of one
    u, v = field.uv(root[:, 0], root[:, 1])
    on_cell_line = lambda w: int(((w == np.floor(w)) & (w % r["cell"] == 0)).sum())
    just_below = lambda w: int((np.nextafter(w, np.float32(np.inf)) == np.ceil(w)).sum() + ((np.ceil(w) - w > 0) & (np.ceil(w) - w < 2e-5)).sum())
    assert on_cell_line(u) >= 4 and on_cell_line(v) >= 4, (on_cell_line(u), on_cell_line(v))       # ... and on a bound-cell line
    assert just_below(u) >= 5 and just_below(v) >= 5                                              # ... and a float or so below one

    for name, (hscale, _, rows, cols) in TE.SCALES.items():
        r = TE.reach_counts("scales_" + name)
        hr, hc = r["table"]
        assert (hr, hc) == (-(-rows // r["cell"]), -(-cols // r["cell"]))
        # the last cell a lookup can reach holds sample rows - 2 (u is clamped below rows - 1): the partial one at cells of 7; where the
        # last cell is the last sample alone (cells of 2 on 33 x 27, cells of 1) that entry is built and never read
        lr, lc = (rows - 2) // r["cell"], (cols - 2) // r["cell"]
        assert (lr, lc) == ((hr - 1, hc - 1) if name == "h0.07" else (hr - 2, hc - 2))
        last_row, last_col = sum(ci == lr for ci, _ in r["cells"]), sum(cj == lc for _, cj in r["cells"])
        assert last_row >= 3 and last_col >= 3, (name, last_row, last_col)                        # bases in the last cells, partial ones
        assert len(r["cells"]) >= min(40, hr * hc // 2), (name, len(r["cells"]))                  # ... and over the whole table
        assert r["corners"]["above_u"] + r["corners"]["above_v"] >= 20 and r["corners"]["below_u"] + r["corners"]["below_v"] >= 8, (name, r["corners"])

    field, root, dof, _ = TE.scene("walls")
    cf = TE.ground_forces("walls")
    arms = np.linalg.norm(cf[:, 20:28], axis=2).max(axis=1) > 1.0, np.linalg.norm(cf[:, 30:38], axis=2).max(axis=1) > 1.0
    assert int((arms[0] | arms[1]).sum()) >= 100          # (Gym bodies 20 .. 27 and 30 .. 37: the links of the two arms) nearly every robot touches its pillar
    assert int((np.linalg.norm(cf[:, list(TE.FEET)], axis=2).sum(axis=1) > 100.0).sum()) >= 100          # ... standing on its feet
