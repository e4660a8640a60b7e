"""TOCABI model compiler and loader.

Turns the robot description the reference task loads through
``gym.load_asset`` (reference: tasks/dyros_dynamic_walk.py:276-293, asset
``assets/mjcf/dyros_tocabi/xml/dyros_tocabi.xml``) into the flat arrays the
HIP kernels and the CPU oracle consume:

* 38 rigid bodies in XML depth-first order (the Gym body index used by
  ``net_contact_force`` and ``apply_rigid_body_force_tensors``),
* 34 *moving* bodies (floating base + 33 hinge links; moving body ``b`` is driven
  by DoF ``b-1``), the four joint-less foot bodies welded into their parent,
* 36 inertial records (mass, COM, inertia about the COM in the owning moving
  body's frame), kept separate so the per-body mass randomisation of
  ``apply_randomizations`` (reference: tasks/base/vec_task.py:519-733) can scale
  each Gym body on its own,
* 61 collision primitives (boxes / cylinders, class ``cls``) in moving-body frames,
* the 8 sole-corner points of the two ``*_Foot_Link`` boxes that enter the contact solve.

The compiled model is committed as ``assets/tocabi_model.json`` (data derived from
the MJCF; the XML itself is not shipped).  ``compile_mjcf`` only runs where the
reference checkout is present (``tools/compile_assets.py``).
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass
from typing import Dict, List

import numpy as np

from . import cbind

ASSET_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets")
MODEL_JSON = os.path.join(ASSET_DIR, "tocabi_model.json")

# the model's fixed sizes, as include/dyros_walk.h has them: 38 Gym rigid bodies (reference: SURVEY appendix A), 34 moving ones (floating base +
# 33 hinge links), 33 DoF, 36 inertial records, and the capacities of the geometry, sole-point and self-collision tables
(NUM_BODIES, NUM_MOVING, NUM_DOF, NUM_INERT, MAX_GEOMS, NUM_FOOT_PTS, MAX_SC_PROXIES, MAX_SC_PAIRS) = (
    cbind.constants("dyros_walk.h", "dw_")["DW_" + n] for n in ("NUM_BODIES", "NUM_MOVING", "NUM_DOF", "NUM_INERT", "MAX_GEOMS", "NUM_FOOT_PTS",
                                                               "MAX_SC_PROXIES", "MAX_SC_PAIRS"))
# links that get a self-collision capsule: (left, right) chains thigh / shank / ankle / foot assembly ...
SC_LEG_BODIES = ("Thigh_Link", "Knee_Link", "AnkleCenter_Link", "Foot_Redundant_Link")
# ... and, second tranche ("leg<->leg, arm<->torso/leg"): upper arm, forearm, hand of each arm and the torso
SC_ARM_BODIES = ("Armlink_Link", "Forearm_Link", "Wrist2_Link")
SC_TORSO_BODY = "Upperbody_Link"
SC_HEAD_BODY = "Head_Link"

# Per-DoF constants the reference hard-codes in the task (not in the MJCF).
# reference: tasks/dyros_dynamic_walk.py:366-372 (armature, damping, velocity)
ARMATURE = [0.614, 0.862, 1.09, 1.09, 1.09, 0.360,
            0.614, 0.862, 1.09, 1.09, 1.09, 0.360,
            0.078, 0.078, 0.078,
            0.18, 0.18, 0.18, 0.18, 0.0032, 0.0032, 0.0032, 0.0032,
            0.0032, 0.0032,
            0.18, 0.18, 0.18, 0.18, 0.0032, 0.0032, 0.0032, 0.0032]
DOF_DAMPING = 0.1
DOF_MAX_VELOCITY = 4.03


def _quat_wxyz_to_mat(q) -> np.ndarray:
    w, x, y, z = [float(v) for v in q]
    n = math.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    return np.array([
        [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
        [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
        [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)],
    ])


def _floats(s, n=None, default=None):
    if s is None:
        return list(default)
    v = [float(t) for t in s.split()]
    if n is not None:
        assert len(v) == n, (s, n)
    return v


def compile_mjcf(xml_path: str) -> Dict:
    """Parse the MJCF into the compiled-model dictionary (plain lists, float64)."""
    import xml.etree.ElementTree as ET

    root = ET.parse(xml_path).getroot()
    world = root.find("worldbody")
    top = world.find("body")

    bodies: List[Dict] = []

    def visit(elem, parent38):
        idx = len(bodies)
        pos = _floats(elem.get("pos"), 3, (0, 0, 0))
        quat = _floats(elem.get("quat"), 4, (1, 0, 0, 0))
        joint = elem.find("joint")
        jtype = None
        axis = [0.0, 0.0, 0.0]
        rng = [0.0, 0.0]
        jname = None
        if joint is not None:
            jtype = joint.get("type", "hinge")
            jname = joint.get("name")
            if jtype == "hinge":
                axis = _floats(joint.get("axis"), 3)
                assert _floats(joint.get("pos"), 3, (0, 0, 0)) == [0.0, 0.0, 0.0]
                rng = _floats(joint.get("range"), 2)
        inertial = elem.find("inertial")
        inert = None
        if inertial is not None:
            m = float(inertial.get("mass"))
            c = _floats(inertial.get("pos"), 3)
            ixx, iyy, izz, ixy, ixz, iyz = _floats(inertial.get("fullinertia"), 6)
            I = np.array([[ixx, ixy, ixz], [ixy, iyy, iyz], [ixz, iyz, izz]])
            iq = inertial.get("quat")
            if iq is not None:
                R = _quat_wxyz_to_mat(_floats(iq, 4))
                I = R @ I @ R.T
            inert = dict(mass=m, com=c, I=I.tolist())
        geoms = []
        for g in elem.findall("geom"):
            if g.get("class") != "cls":
                continue
            gtype = g.get("type")
            assert gtype in ("box", "cylinder"), gtype
            size = _floats(g.get("size"))
            geoms.append(dict(type=gtype, pos=_floats(g.get("pos"), 3, (0, 0, 0)),
                              quat=_floats(g.get("quat"), 4, (1, 0, 0, 0)), size=size))
        bodies.append(dict(name=elem.get("name"), parent=parent38, pos=pos, quat=quat,
                           jtype=jtype, jname=jname, axis=axis, range=rng,
                           inertial=inert, geoms=geoms))
        for child in elem.findall("body"):
            visit(child, idx)

    visit(top, -1)
    assert len(bodies) == NUM_BODIES, len(bodies)

    # --- moving bodies: the free root and every hinge body, in depth-first order ---
    moving_of_body = [-1] * NUM_BODIES          # gym body -> moving body that carries it
    T_in_moving = [None] * NUM_BODIES           # (R, p) of gym body frame in its moving body's frame
    mv_gym, mv_parent, mv_pos, mv_rot0, mv_axis, mv_range, dof_names = [], [], [], [], [], [], []
    for i, b in enumerate(bodies):
        R = _quat_wxyz_to_mat(b["quat"])
        p = np.array(b["pos"])
        if b["jtype"] is not None:
            m = len(mv_gym)
            moving_of_body[i] = m
            T_in_moving[i] = (np.eye(3), np.zeros(3))
            mv_gym.append(i)
            mv_parent.append(-1 if b["parent"] < 0 else moving_of_body[b["parent"]])
            if b["parent"] >= 0:
                # parent gym body may itself be welded: compose
                Rp, pp = T_in_moving[b["parent"]]
                mv_pos.append((pp + Rp @ p).tolist())
                mv_rot0.append((Rp @ R).tolist())
            else:
                mv_pos.append(p.tolist())
                mv_rot0.append(R.tolist())
            ax = np.array(b["axis"])
            if b["jtype"] == "hinge":
                ax = ax / np.linalg.norm(ax)
                dof_names.append(b["jname"])
            mv_axis.append(ax.tolist())
            mv_range.append(b["range"])
        else:
            # a jointless body (the four foot bodies) sits on its parent with no offset and no rotation: the rigid-body state tensor
            # (include/dyros_bodies.h) gives it its carrier's pose
            assert not np.any(p) and np.array_equal(R, np.eye(3)), (b["name"], b["pos"], b["quat"])
            Rp, pp = T_in_moving[b["parent"]]
            moving_of_body[i] = moving_of_body[b["parent"]]
            T_in_moving[i] = (Rp @ R, pp + Rp @ p)
    assert len(mv_gym) == NUM_MOVING and len(dof_names) == NUM_DOF

    # depth of every moving body (root = 0)
    depth = [0] * NUM_MOVING
    for m in range(1, NUM_MOVING):
        depth[m] = depth[mv_parent[m]] + 1

    # --- inertial records ---
    inert_mv, inert_gym, inert_mass, inert_com, inert_I = [], [], [], [], []
    for i, b in enumerate(bodies):
        if b["inertial"] is None:
            continue
        R, p = T_in_moving[i]
        inert_mv.append(moving_of_body[i])
        inert_gym.append(i)
        inert_mass.append(b["inertial"]["mass"])
        inert_com.append((p + R @ np.array(b["inertial"]["com"])).tolist())
        inert_I.append((R @ np.array(b["inertial"]["I"]) @ R.T).tolist())
    assert len(inert_mv) == NUM_INERT

    # --- collision primitives ---
    geoms = []
    foot_pts = []
    for i, b in enumerate(bodies):
        R, p = T_in_moving[i]
        for g in b["geoms"]:
            Rg = R @ _quat_wxyz_to_mat(g["quat"])
            pg = p + R @ np.array(g["pos"])
            if g["type"] == "box":
                size = list(g["size"]) + [0.0] * (3 - len(g["size"]))
                gt = 0
            else:
                size = [g["size"][0], g["size"][1], 0.0]   # radius, half height (axis = local z)
                gt = 1
            is_sole = b["name"] in ("L_Foot_Link", "R_Foot_Link")
            geoms.append(dict(type=gt, moving=moving_of_body[i], gym=i, pos=pg.tolist(),
                              rot=Rg.tolist(), size=size, sole=int(is_sole)))
            if is_sole:
                hx, hy, hz = size
                for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                    c = pg + Rg @ np.array([sx * hx, sy * hy, -hz])
                    foot_pts.append(dict(moving=moving_of_body[i], gym=i, pos=c.tolist()))
    assert len(foot_pts) == NUM_FOOT_PTS

    names = [b["name"] for b in bodies]
    # --- self-collision capsule proxies: the largest collision primitive of each listed link.  cylinder -> capsule
    #     (same radius, same half length); box -> capsule along its longest axis, radius = second-longest half
    #     extent, half length = longest - radius.  Pairs: every left-leg proxy against every right-leg proxy.
    sc_proxies, side_of = [], []
    for side in ("L_", "R_"):
        for suffix in SC_LEG_BODIES:
            i = names.index(side + suffix)
            R, p = T_in_moving[i]
            best, vol = None, -1.0
            for g in bodies[i]["geoms"]:
                sz = g["size"]
                v = (8 * sz[0] * sz[1] * sz[2]) if g["type"] == "box" else (3.14159 * sz[0] * sz[0] * 2 * sz[1])
                if v > vol:
                    best, vol = g, v
            Rg = R @ _quat_wxyz_to_mat(best["quat"])
            pg = p + R @ np.array(best["pos"])
            if best["type"] == "cylinder":
                rad, half, ax = best["size"][0], best["size"][1], Rg[:, 2]
            else:
                order = np.argsort(best["size"])[::-1]
                rad = best["size"][order[1]]
                half = max(best["size"][order[0]] - rad, 0.0)
                ax = Rg[:, order[0]]
            sc_proxies.append(dict(moving=moving_of_body[i], gym=i, p0=(pg - half * ax).tolist(), p1=(pg + half * ax).tolist(),
                                   radius=float(rad)))
            side_of.append(side)
    nl = len(SC_LEG_BODIES)
    sc_pairs = [[a, nl + b] for a in range(nl) for b in range(nl)]

    # second tranche: arms and torso.  A link with several primitives strung along one line (forearm: two cylinders; torso:
    # a stack of boxes) gets ONE capsule around all of them: axis = the line through the two outermost primitive centres,
    # half length to the outermost primitive ends, radius = the largest cross-section radius.
    def span_capsule(i):
        R, p = T_in_moving[i]
        cs, rads, ext = [], [], []
        for g in bodies[i]["geoms"]:
            Rg = R @ _quat_wxyz_to_mat(g["quat"])
            cs.append(p + R @ np.array(g["pos"]))
            sz = list(g["size"]) + [0.0] * (3 - len(g["size"]))
            if g["type"] == "cylinder":
                rads.append((sz[0], sz[1], Rg[:, 2]))
            else:
                rads.append((None, sz, Rg))
        cs = np.array(cs)
        if len(cs) == 1:
            ax = rads[0][2] if rads[0][0] is not None else rads[0][2][:, int(np.argmax(rads[0][1]))]
        else:
            d = cs[:, None, :] - cs[None, :, :]
            i0, i1 = np.unravel_index(np.argmax((d ** 2).sum(-1)), d.shape[:2])
            ax = cs[i1] - cs[i0]
        ax = ax / np.linalg.norm(ax)
        lo, hi, rad = np.inf, -np.inf, 0.0
        for c, (r, h, A) in zip(cs, rads):
            t = float((c - cs[0]) @ ax)
            if r is not None:                       # cylinder: half height along its own axis, projected
                e = abs(float(A @ ax)) * h + np.sqrt(max(0.0, 1 - float(A @ ax) ** 2)) * r
                rr = r
            else:                                   # box: extent along the capsule axis, radius = second-largest half extent across it
                e = float(sum(abs(float(A[:, k] @ ax)) * h[k] for k in range(3)))
                across = sorted((h[k] for k in range(3) if abs(float(A[:, k] @ ax)) < 0.9), reverse=True)
                rr = across[0] if len(across) < 2 else across[1] if len(across) == 3 else across[0]
                rr = max(across[-1], min(across[0], rr))
            lo, hi, rad = min(lo, t - e), max(hi, t + e), max(rad, rr)
        lo, hi = lo + rad, hi - rad                 # the caps take one radius at each end
        if hi < lo:
            lo = hi = 0.5 * (lo + hi)
        return dict(moving=moving_of_body[i], gym=i, p0=(cs[0] + lo * ax).tolist(), p1=(cs[0] + hi * ax).tolist(), radius=float(rad))

    idx = {}
    for side in ("L_", "R_"):
        for suffix in SC_ARM_BODIES:
            idx[side + suffix] = len(sc_proxies)
            sc_proxies.append(span_capsule(names.index(side + suffix)))
    idx[SC_TORSO_BODY] = len(sc_proxies)
    sc_proxies.append(span_capsule(names.index(SC_TORSO_BODY)))
    thigh = {"L_": 0, "R_": nl}
    for side in ("L_", "R_"):
        for part in ("Forearm_Link", "Wrist2_Link"):
            sc_pairs.append([idx[side + part], idx[SC_TORSO_BODY]])          # forearm / hand against the torso
            sc_pairs.append([idx[side + part], thigh[side]])                 # ... and against the thigh of the same side
        sc_pairs.append([idx[side + "Armlink_Link"], idx[SC_TORSO_BODY]])    # upper arm against the torso
    sc_pairs += [[idx["L_Forearm_Link"], idx["R_Forearm_Link"]], [idx["L_Wrist2_Link"], idx["R_Wrist2_Link"]],
                 [idx["L_Wrist2_Link"], idx["R_Forearm_Link"]], [idx["L_Forearm_Link"], idx["R_Wrist2_Link"]]]
    # third tranche (towards the reference's filter 0, tasks/dyros_dynamic_walk.py:354): each hand against the thigh of the OTHER
    # side.  With it the pair table of the kernels (32) is full.  A head capsule does not fit the octet kernels' budget of four
    # proxies per lane (its lane already carries an arm and the torso); what is still absent is listed in DESIGN.md section 2
    other = {"L_": "R_", "R_": "L_"}
    for side in ("L_", "R_"):
        sc_pairs.append([idx[side + "Wrist2_Link"], thigh[other[side]]])
    # fourth tranche (round 5; the kernels' pair table holds 64 since the detection tests pairs in rounds of eight, dw_oct.h): a head
    # capsule -- the 16th proxy, the table of proxies is full with it -- against forearms and hands; upper arm against the thigh of its
    # side, forearm against the thigh of the other side, hand against the shank of its side; upper arm against the other arm's upper
    # arm, forearm and hand.  Still absent from the reference's filter 0: the waist links and the neck (no proxy left), the foot
    # boxes as boxes.
    knee = {"L_": 1, "R_": nl + 1}
    idx[SC_HEAD_BODY] = len(sc_proxies)
    sc_proxies.append(span_capsule(names.index(SC_HEAD_BODY)))
    for side in ("L_", "R_"):
        for part in ("Forearm_Link", "Wrist2_Link"):
            sc_pairs.append([idx[SC_HEAD_BODY], idx[side + part]])
    for side in ("L_", "R_"):
        sc_pairs.append([idx[side + "Armlink_Link"], thigh[side]])
        sc_pairs.append([idx[side + "Forearm_Link"], thigh[other[side]]])
        sc_pairs.append([idx[side + "Wrist2_Link"], knee[side]])
    sc_pairs.append([idx["L_Armlink_Link"], idx["R_Armlink_Link"]])
    for side in ("L_", "R_"):
        sc_pairs.append([idx[side + "Armlink_Link"], idx[other[side] + "Forearm_Link"]])
        sc_pairs.append([idx[side + "Wrist2_Link"], idx[other[side] + "Armlink_Link"]])

    # Proxy ORDER (free: pairs name proxies by index).  The kernels' detection keeps proxy p in octet lane p & 7 as class p >> 3 and
    # tests the pairs in rounds of eight with uniform classes (csrc/dw_quad_model.h QHot::scround): order the proxies so that the three
    # class combinations need the fewest rounds -- first split of the 16 proxies in two classes of eight, in lexicographic order, that
    # attains the minimum (TOCABI: 6 rounds for 47 pairs; legs-first order needs 7).
    if len(sc_proxies) > 8:
        import itertools
        import math
        best = None
        for c0 in itertools.combinations(range(len(sc_proxies)), 8):
            s0 = set(c0)
            n00 = sum(1 for a, b in sc_pairs if a in s0 and b in s0)
            n11 = sum(1 for a, b in sc_pairs if a not in s0 and b not in s0)
            r = math.ceil(n00 / 8) + math.ceil(n11 / 8) + math.ceil((len(sc_pairs) - n00 - n11) / 8)
            if best is None or r < best[0]:
                best = (r, c0)
        order = list(best[1]) + [p for p in range(len(sc_proxies)) if p not in set(best[1])]
        new_of = {old: new for new, old in enumerate(order)}
        sc_proxies = [sc_proxies[old] for old in order]
        sc_pairs = [[new_of[a], new_of[b]] for a, b in sc_pairs]

    model = dict(
        body_names=names,
        dof_names=dof_names,
        body_parent=[b["parent"] for b in bodies],
        body_moving=moving_of_body,
        mv_gym=mv_gym, mv_parent=mv_parent, mv_depth=depth,
        mv_pos=mv_pos, mv_rot0=mv_rot0, mv_axis=mv_axis,
        dof_lower=[min(r) for r in mv_range[1:]],
        dof_upper=[max(r) for r in mv_range[1:]],
        inert_mv=inert_mv, inert_gym=inert_gym, inert_mass=inert_mass,
        inert_com=inert_com, inert_I=inert_I,
        geoms=geoms, foot_pts=foot_pts,
        left_foot_idx=names.index("L_Foot_Link"),
        right_foot_idx=names.index("R_Foot_Link"),
        pelvis_idx=names.index("base_link"),
        root_pos=bodies[0]["pos"],
        sc_proxies=sc_proxies, sc_pairs=sc_pairs,
    )
    return model


# ---------------------------------------------------------------------------------------
# include/dyros_walk.h :: DwModel and the two structs it embeds, read from the header (cbind.py)
# ---------------------------------------------------------------------------------------
DwGeom, DwCapsule, DwModel = (cbind.structs("dyros_walk.h", "dw_")[n] for n in ("DwGeom", "DwCapsule", "DwModel"))


@dataclass
class TocabiModel:
    """Compiled model with numpy views plus the packed C struct."""
    d: Dict

    def __getattr__(self, k):
        try:
            return self.__dict__["d"][k]
        except KeyError as e:
            raise AttributeError(k) from e

    @property
    def nominal_total_mass(self) -> float:
        return float(sum(self.d["inert_mass"]))

    def non_feet_idxs(self) -> List[int]:
        """reference: tasks/dyros_dynamic_walk.py:320-324"""
        return [i for i in range(NUM_BODIES)
                if i not in (self.d["left_foot_idx"], self.d["right_foot_idx"])]

    def to_c(self) -> DwModel:
        d = self.d
        m = DwModel()
        for i in range(NUM_MOVING):
            m.mv_parent[i] = d["mv_parent"][i]
            m.mv_gym[i] = d["mv_gym"][i]
            m.mv_depth[i] = d["mv_depth"][i]
            for k in range(3):
                m.mv_pos[i][k] = d["mv_pos"][i][k]
                m.mv_axis[i][k] = d["mv_axis"][i][k]
            for r in range(3):
                for c in range(3):
                    m.mv_rot0[i][3 * r + c] = d["mv_rot0"][i][r][c]
        for j in range(NUM_DOF):
            m.dof_lower[j] = d["dof_lower"][j]
            m.dof_upper[j] = d["dof_upper"][j]
            m.dof_vmax[j] = DOF_MAX_VELOCITY
        for i in range(NUM_INERT):
            m.inert_mv[i] = d["inert_mv"][i]
            m.inert_gym[i] = d["inert_gym"][i]
            m.inert_mass[i] = d["inert_mass"][i]
            I = d["inert_I"][i]
            for k in range(3):
                m.inert_com[i][k] = d["inert_com"][i][k]
            vals = (I[0][0], I[1][1], I[2][2], I[0][1], I[0][2], I[1][2])
            for k in range(6):
                m.inert_I[i][k] = vals[k]
        geoms = d["geoms"]
        assert len(geoms) <= MAX_GEOMS
        m.num_geoms = len(geoms)
        for i, g in enumerate(geoms):
            cg = m.geoms[i]
            cg.type, cg.moving, cg.gym, cg.sole = g["type"], g["moving"], g["gym"], g["sole"]
            for k in range(3):
                cg.pos[k] = g["pos"][k]
                cg.size[k] = g["size"][k]
            for r in range(3):
                for c in range(3):
                    cg.rot[3 * r + c] = g["rot"][r][c]
        for i, f in enumerate(d["foot_pts"]):
            m.foot_mv[i] = f["moving"]
            m.foot_gym[i] = f["gym"]
            for k in range(3):
                m.foot_pos[i][k] = f["pos"][k]
        m.left_foot_gym = d["left_foot_idx"]
        m.right_foot_gym = d["right_foot_idx"]
        m.pelvis_gym = d["pelvis_idx"]
        prox, pairs = d.get("sc_proxies", []), d.get("sc_pairs", [])
        assert len(prox) <= MAX_SC_PROXIES and len(pairs) <= MAX_SC_PAIRS
        m.num_sc_proxies, m.num_sc_pairs = len(prox), len(pairs)
        for i, c in enumerate(prox):
            m.sc_proxy[i].moving, m.sc_proxy[i].gym, m.sc_proxy[i].radius = c["moving"], c["gym"], c["radius"]
            for k in range(3):
                m.sc_proxy[i].p0[k] = c["p0"][k]
                m.sc_proxy[i].p1[k] = c["p1"][k]
        for i, (a, b) in enumerate(pairs):
            m.sc_pair[i][0], m.sc_pair[i][1] = a, b
        return m


def load_model(path: str = MODEL_JSON) -> TocabiModel:
    with open(path) as f:
        return TocabiModel(json.load(f))
