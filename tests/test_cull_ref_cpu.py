"""tests/cull_ref.py against brute force and known answers: the reference the culling bounds are tested against (DESIGN.md
section 5, "Direct tests of the culling bounds") must itself be right.  Dense sampling: a leaf is 1-Lipschitz, so with samples dt
apart the true infimum lies in [min over samples - dt / 2, min over samples]; the reference must too, and -- being a value at an
evaluated parameter -- can never be below the truth."""
import numpy as np
import pytest

import cull_ref as R
import scene_f64
import scenes

LEAVES = [
    ("sphere", R.SPHERE, [0.3, -0.2, 0.5, 0.7]),
    ("sphere r=0", R.SPHERE, [0.3, -0.2, 0.5, 0.0]),
    ("sphere r<0", R.SPHERE, [0.3, -0.2, 0.5, -0.25]),
    ("box", R.BOX, [0.3, -0.2, 0.5, 0.6, 0.2, 0.9]),
    ("flat box", R.BOX, [0.3, -0.2, 0.5, 0.6, 0.0, 0.9]),
    ("box h<0", R.BOX, [0.3, -0.2, 0.5, 0.6, -0.1, 0.9]),
    ("box all h<0", R.BOX, [0.3, -0.2, 0.5, -0.3, -0.1, -0.2]),
    ("cylinder", R.CYLINDER, [0.3, -0.2, 0.5, 0.4, 0.8]),
    ("disc", R.CYLINDER, [0.3, -0.2, 0.5, 0.4, 0.0]),
    ("cylinder r<0", R.CYLINDER, [0.3, -0.2, 0.5, -0.2, 0.8]),
]


def _random_rays(rng, n, centre):
    """Origins inside, near and far; directions towards the leaf, past it, away from it, axis-parallel and with tiny components."""
    o = centre + rng.normal(size=(n, 3)) * rng.choice([0.2, 1.0, 4.0], size=(n, 1))
    target = centre + rng.normal(size=(n, 3)) * rng.choice([0.0, 0.5, 1.5], size=(n, 1))
    d = target - o
    d[::7] *= -1.0                                               # pointing away
    axis = np.eye(3)[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], size=(n, 1))
    d[::5] = axis[::5]                                           # axis-parallel: two exact zeros
    d[1::11, 0] = 1e-20                                          # a component that is all but zero
    d[2::11, 2] = -1e-42
    d[np.linalg.norm(d, axis=1) == 0] = (0.0, 1.0, 0.0)
    return o, d * rng.choice([1e-3, 1.0, 1e3], size=(n, 1))


@pytest.mark.parametrize("name,op,a", LEAVES, ids=[x[0] for x in LEAVES])
def test_closest_approach_against_dense_sampling(name, op, a):
    rng = np.random.default_rng(5)
    a = np.array(a)
    o, d = _random_rays(rng, 400, a[:3])
    inf, t = R.closest_approach(op, a, o, d)
    dh = R.unit(d)
    far = np.linalg.norm(a[:3] - o, axis=1) + 4.0
    K = 4001
    ts = np.linspace(0.0, 1.0, K)[None, :] * far[:, None]
    dense = R.leaf_along(op, a, o, dh, ts).min(axis=1)
    dt = far / (K - 1)
    assert np.all(t >= 0.0)
    np.testing.assert_allclose(R.leaf_along(op, a, o, dh, t), inf, rtol=0, atol=0)        # attained where it says
    assert np.all(inf <= dense + 1e-12), (name, float((inf - dense).max()))
    assert np.all(inf >= dense - 0.5 * dt - 1e-12), (name, float((dense - inf).max()))
    # and it is a local minimum of the convex value: stepping either way does not go lower
    for s in (-1e-6, 1e-6, -1e-3, 1e-3):
        assert np.all(R.leaf_along(op, a, o, dh, np.maximum(t + s, 0.0)) >= inf - 1e-13)


def test_closest_approach_known_answers():
    box = np.array([1.0, 2.0, 3.0, 0.5, 0.25, 0.75])
    sph = np.array([1.0, 2.0, 3.0, 0.5])
    cyl = np.array([1.0, 2.0, 3.0, 0.5, 0.25])

    def ca(op, a, o, d):
        v, t = R.closest_approach(op, a, np.array([o], dtype=float), np.array([d], dtype=float))
        return float(v[0]), float(t[0])

    # axis-parallel rays passing a face at distance 0.3, an edge at (0.3, 0.4) and a ray through a corner's diagonal
    v, t = ca(R.BOX, box, (-5, 2.0, 3.0 + 0.75 + 0.3), (2, 0, 0))
    assert v == pytest.approx(0.3, abs=1e-12) and 5.5 - 1e-9 <= t <= 6.5 + 1e-9
    v, t = ca(R.BOX, box, (-5, 2.25 + 0.4, 3.75 + 0.3), (1, 0, 0))
    assert v == pytest.approx(0.5, abs=1e-12)
    v, t = ca(R.BOX, box, (1.5 + 1, 2.25 + 1 - 2, 3.75 + 1), (0, 1, 0))                 # passes the corner at (1, ., 1)
    assert v == pytest.approx(np.sqrt(2.0), abs=1e-12) and 0.5 - 1e-6 <= t <= 1.0 + 1e-6
    # origins inside: the value at the origin, or deeper along the ray
    assert ca(R.SPHERE, sph, (1, 2, 3), (0, 0, 1)) == (-0.5, 0.0)
    assert ca(R.SPHERE, sph, (1.25, 2, 3), (-1e-3, 0, 0)) == pytest.approx((-0.5, 0.25), abs=1e-12)
    v, t = ca(R.BOX, box, (1, 2, 3), (1, 0, 0))
    assert v == -0.25 and t <= 0.25 + 1e-9
    v, t = ca(R.BOX, box, (1.4, 2.2, 3), (-1, 0, 0))                                  # towards the middle: as deep as x and z allow
    assert v == pytest.approx(-0.05, abs=1e-12)
    v, t = ca(R.CYLINDER, cyl, (1, 2, 3), (0, 1, 0))
    assert v == -0.25
    # pointing away: the value at the origin
    assert ca(R.SPHERE, sph, (3, 2, 3), (1e3, 0, 0)) == pytest.approx((1.5, 0.0), abs=1e-15)
    assert ca(R.BOX, box, (3, 2, 3), (1, 1e-20, 0)) == pytest.approx((1.5, 0.0), abs=1e-15)
    assert ca(R.CYLINDER, cyl, (1, 4, 3), (0, 1, 0)) == pytest.approx((1.75, 0.0), abs=1e-15)
    # cylinder: a ray along the axis direction beside the rim, a ray across the cap's rim
    v, t = ca(R.CYLINDER, cyl, (1.8, -5, 3), (0, 1, 0))
    assert v == pytest.approx(0.3, abs=1e-12)
    v, t = ca(R.CYLINDER, cyl, (-5, 2.25 + 0.4, 3), (1, 0, 0))
    assert v == pytest.approx(0.4, abs=1e-12)
    v, t = ca(R.CYLINDER, cyl, (-5, 2.25 + 0.4, 3.5 + 0.3), (1, 0, 0))                  # past the rim: radial 0.3, axial 0.4
    assert v == pytest.approx(0.5, abs=1e-12)
    # planes: level or rising -> the origin's value; descending -> unbounded below
    pl = np.array([0.0, 2.0, 0.0, 1.0])
    assert ca(R.PLANE, pl, (0, 1, 0), (1, 0, 0)) == (3.0, 0.0)
    assert ca(R.PLANE, pl, (0, 1, 0), (1, 1, 0)) == (3.0, 0.0)
    assert ca(R.PLANE, pl, (0, 1, 0), (1, -1e-9, 0)) == (-np.inf, np.inf)


def test_zone_tests_against_dense_sampling_and_tangents():
    rng = np.random.default_rng(6)
    c, h = np.array([0.3, -0.2, 0.5]), np.array([0.6, 0.2, 0.9])
    o, d = _random_rays(rng, 600, c)
    dh = R.unit(d)
    far = np.linalg.norm(c - o, axis=1) + 4.0
    ts = np.linspace(0.0, 1.0, 4001)[None, :] * far[:, None]
    box_sdf = R.leaf_along(R.BOX, np.concatenate([c, h]), o, dh, ts).min(axis=1)
    ball_sdf = R.leaf_along(R.SPHERE, np.concatenate([c, [0.8]]), o, dh, ts).min(axis=1)
    dt = far / 4000
    for sdf, meets in ((box_sdf, R.meets_box(c, h, o, d)), (ball_sdf, R.meets_ball(c, 0.8, o, d))):
        assert np.all(meets[sdf <= 0.0])
        assert not np.any(meets[sdf > 0.5 * dt])
        assert meets.any() and not meets.all()
    # tangents: exactly on the boundary counts as meeting (the zone is closed); a hair outside does not
    o1 = np.array([[-5.0, c[1] + h[1], c[2]]])
    assert R.meets_box(c, h, o1, [[1.0, 0.0, 0.0]])[0] and not R.meets_box(c, h, o1 + [0, 1e-12, 0], [[1.0, 0.0, 0.0]])[0]
    assert not R.meets_box(c, h, o1, [[-1.0, 0.0, 0.0]])[0]                                # behind the origin
    assert R.meets_box(c, h, [c], [[0.0, 0.0, 1e-30]])[0]                                  # origin inside
    o2 = np.array([[-5.0, c[1] + 0.8, c[2]]])
    assert R.meets_ball(c, 0.8, o2, [[1.0, 0.0, 0.0]])[0] and not R.meets_ball(c, 0.8, o2 + [0, 1e-12, 0], [[1.0, 0.0, 0.0]])[0]
    assert not R.meets_ball(c, 0.8, o2, [[-1.0, 0.0, 0.0]])[0]


def test_cull_margin_and_zones():
    M = R.cull_margin((1.0, -2.0, 3.0), 0.5, (4.0, 0.0, -1.0), 0.01, 0.25)
    assert M == pytest.approx((0.01 + 0.25) * 1.01 + 1e-4 * (1 + 6 + 0.5 + 5 + 0.25), rel=1e-15)
    assert R.cull_margin((0, 0, 0), 0.0, (0, 0, 0), -1.0, 0.0) == pytest.approx(1e-4, rel=1e-15)       # a negative min_dist counts as 0
    kind, c, rad = R.zone(R.SPHERE, [1.0, -2.0, 3.0, -0.5], (0, 0, 0), 0.01, 0.0)
    assert kind == "ball" and rad == pytest.approx(R.cull_margin((1, -2, 3), 0.0, (0, 0, 0), 0.01, 0.0))
    kind, c, hz = R.zone(R.CYLINDER, [0.0, 0.0, 0.0, 0.5, 0.25], (0, 0, 0), 0.0, 0.0)
    assert kind == "box" and np.allclose(hz - R.cull_margin((0, 0, 0), 1.25, (0, 0, 0), 0.0, 0.0), [0.5, 0.25, 0.5], atol=1e-15)
    assert np.all(R.zone(R.BOX, [0, 0, 0, 1, 1, 1], (0, 0, 0), 0.1, 0.0, shrink=1e-3)[2] < R.zone(R.BOX, [0, 0, 0, 1, 1, 1], (0, 0, 0), 0.1, 0.0)[2])


@pytest.mark.parametrize("scene", ["g8", "g8x", "g32s", "ext_mix", "xform_mix"])
def test_scene_infimum_against_dense_sampling(oracle, scene):
    nodes, root = {**scenes.SCENES, **scenes.EXT_SCENES}[scene]()
    cc, words = oracle.serialize(nodes, root)
    words = np.asarray(words, dtype=np.uint32)
    rng = np.random.default_rng(7)
    o, d = _random_rays(rng, 96, np.zeros(3))
    o = o + rng.normal(size=o.shape)
    inf, t = R.scene_infimum(cc, words, o, d)
    dh = R.unit(d)
    np.testing.assert_array_equal(scene_f64.map_scene(cc, words, 100.0, o + t[:, None] * dh), inf)      # a value that is attained
    assert np.all(inf <= scene_f64.map_scene(cc, words, 100.0, o))                                        # t = 0 is among them
    K = 3001
    ts = np.linspace(0.0, 30.0, K)
    dense = np.stack([scene_f64.map_scene(cc, words, 100.0, o + x * dh) for x in ts], axis=1).min(axis=1)
    # every operator is 1-Lipschitz in its operands except a Scale scope's factor; the named scenes' values move by at most 2 dt
    # between samples (plane normals up to |n| = 1.02, scales below 1)
    lip = 2.0
    assert np.all(inf <= dense + lip * 0.5 * (30.0 / (K - 1))), float((inf - dense).max())
    assert (inf <= dense + 1e-9).mean() > 0.9                                 # and nearly always at least as low as the samples


def test_commands_reports_open_scopes(oracle):
    cc, words = oracle.serialize(*scenes.xform_mix())
    cmds = R.commands(cc, np.asarray(words, dtype=np.uint32))
    assert len(cmds) == cc and [c[2] for c in cmds if c[0] in (0, 1, 10)] == [2, 1, 1, 3, 3, 1]
    assert R.words_of((0, [0, 0, 0, 1.0]))[0] == 1
