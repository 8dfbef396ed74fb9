"""The anchored pruning threshold against binary64 geometry, without a GPU (rm_kernel_v5.h "Pruning", anchored first step).

The claim the march relies on: with (a, F_a) any point of the launch and the value computed there, the threshold the step hands to
the culling at q bounds the value computed at q,  thr >= |F(q)| + E(q),  E the evaluation error bound of "Pruning".  Here F is
tests/scene_f64.py's, the computed F_a is modelled as ANY binary32 number within E(a) of it -- the rounded value, and the two
ends of the interval, the lower one being the worst case --, and the formulas are tests/anchor_ref.py's binary32 restatement.
Pairs on and off a common start sphere, seeded; g32, g64, the balanced tree, a scene 1000 units from the origin and one of
degenerate radii."""
import numpy as np
import pytest

import anchor_ref as A
import scene_f64
import scenes
from test_cull_tables_cpu import decode

F = np.float32
N_PAIRS = 3000
MAX_DIST = 100.0


def camera_positions(oracle, centre):
    """the still camera and one ten times as far, about the program's centre"""
    out = []
    for radius in (5.0, 50.0):
        _, pos, _, _ = oracle.orbit_uniforms((64.0, 64.0), target=tuple(centre), radius=radius, events=scenes.STILL_CAMERA_EVENTS)
        out.append(np.array(pos, dtype=F))
    return out


@pytest.mark.parametrize("name", A.PAIR_PROGRAMS)
def test_threshold_bounds_the_value_at_q(oracle, name):
    cc, w, centre = A.program(oracle, name)
    scene_scale = decode(cc, w)["scene_scale"]
    rng = np.random.default_rng(2200 + A.PAIR_PROGRAMS.index(name))
    head = np.inf
    for ro in camera_positions(oracle, centre):
        ps = A.prune_scale(scene_scale, ro)
        f0 = float(scene_f64.map_scene(cc, w, MAX_DIST, ro[None])[0])
        pr = A.pairs(ro, centre, abs(f0), rng, N_PAIRS)
        a, q = pr[:, 0], pr[:, 1]
        fa, fq = scene_f64.map_scene(cc, w, MAX_DIST, a), scene_f64.map_scene(cc, w, MAX_DIST, q)
        ea, eq = A.eval_error(ps, a), A.eval_error(ps, q)
        need = np.abs(fq) + eq
        # the value the device may have computed at a: anything within E(a) of F(a)
        for label, sd in (("rounded", fa), ("F - E", fa - ea), ("F + E", fa + ea), ("|F| - E", np.sign(fa) * np.maximum(np.abs(fa) - ea, 0.0))):
            sd32 = sd.astype(F)
            # (rounding to binary32 must not leave the interval on the side that matters: round |sd| towards zero)
            up = np.abs(sd32.astype(np.float64)) > np.abs(sd)
            sd32 = np.where(up, np.nextafter(sd32, F(0.0)), sd32).astype(F)
            thr = A.threshold(q, a, sd32, ps).astype(np.float64)
            k = int(np.argmin(thr - need))
            assert np.all(thr >= need), "%s, camera %s, F_a %s: pair %d a %s q %s: thr %.9g < |F(q)| + E = %.9g" % (
                name, ro.tolist(), label, k, a[k].tolist(), q[k].tolist(), thr[k], need[k])
            head = min(head, float(((thr - need) / float(ps)).min()))
            # ... and it is a threshold worth having: within 2.1 (|F_a| + |q - a|_1) + margins of nothing
            l1 = np.abs(q.astype(np.float64) - a.astype(np.float64)).sum(axis=1)
            assert np.all(thr <= (np.abs(sd32) + l1) * 1.0001 + 1.0e-5 * (float(ps) + np.abs(a).sum(axis=1) + np.abs(q).sum(axis=1)))
        # the minimum with the camera's own bound keeps whichever is smaller
        cam = F(abs(f0)) * F(2.00002)
        tb = A.anchor_thr_base(cam, q, a, A.anchor_reach(a, fa.astype(F), ps))
        assert np.all(tb <= cam) and np.any(tb < cam)
    print("%s: smallest (thr - |F(q)| - E(q)) / prune_scale %.3g" % (name, head))
    assert head >= 0.0


def test_on_the_start_sphere_the_anchor_beats_the_camera(oracle):
    """what the rule is for: on g32's start sphere, neighbours a few pixels apart get a threshold far below 2 |f0|"""
    cc, w, centre = A.program(oracle, "g32")
    ro = camera_positions(oracle, centre)[0]
    ps = A.prune_scale(decode(cc, w)["scene_scale"], ro)
    f0 = float(scene_f64.map_scene(cc, w, MAX_DIST, ro[None])[0])
    pr = A.pairs(ro, centre, f0, np.random.default_rng(2210), 900)[:300]
    a, q = pr[:, 0], pr[:, 1]
    near = np.abs(q.astype(np.float64) - a).sum(axis=1) < 0.2
    assert near.sum() > 100
    thr = A.threshold(q[near], a[near], scene_f64.map_scene(cc, w, MAX_DIST, a[near]).astype(F), ps)
    assert f0 > 2.5 and np.median(thr) < 0.5 * f0, (f0, float(np.median(thr)))


def test_non_finite_inputs_never_give_a_finite_threshold(oracle):
    cc, w, centre = A.program(oracle, "g32")
    ro = camera_positions(oracle, centre)[0]
    ps = A.prune_scale(decode(cc, w)["scene_scale"], ro)
    rng = np.random.default_rng(2220)
    pr = A.pairs(ro, centre, 3.0, rng, 600)
    sd = scene_f64.map_scene(cc, w, MAX_DIST, pr[:, 0]).astype(F)
    cam = F(6.03)
    bad = A.poisoned(pr, rng)
    for label, a, q, s in (("point", bad[:, 0], bad[:, 1], sd),
                           ("value nan", pr[:, 0], pr[:, 1], np.full_like(sd, np.nan)),
                           ("value inf", pr[:, 0], pr[:, 1], np.full_like(sd, np.inf)),
                           ("value -inf", pr[:, 0], pr[:, 1], np.full_like(sd, -np.inf))):
        thr = A.threshold(q, a, s, ps)
        assert not np.any(np.isfinite(thr)), label
        assert not np.any(thr == -np.inf), label
        # under a finite bound from the camera that bound stays, bit for bit (a NaN position term of q aside: the step's own)
        tb = A.anchor_thr_base(cam, q, a, A.anchor_reach(a, s, ps))
        assert np.all(tb == cam), label
    # no anchor yet (aT = +inf), a NaN bound from the camera (f0 NaN)
    assert np.all(A.anchor_thr_base(cam, pr[:, 1], np.zeros_like(pr[:, 0]), A.INF) == cam)
    good = A.anchor_reach(pr[:, 0], sd, ps)
    assert np.all(np.isnan(A.anchor_thr_base(F(np.nan), pr[:, 1], pr[:, 0], good)))
    assert np.all(np.isfinite(A.threshold(pr[:, 1], pr[:, 0], sd, ps)))     # (the inputs were worth poisoning)
