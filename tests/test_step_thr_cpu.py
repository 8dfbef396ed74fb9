"""The march step's threshold with its position term bounded along the ray (rm_kernel_v5.h "Pruning", the position term along a
ray), without a GPU: tests/step_thr_ref.py's binary32 restatement against the old expression and against binary64 geometry.

new >= old        along marched rays of g32, g64, the balanced tree, a scene 1000 units out and one of degenerate radii, at the
                  hand-out (plain and anchored) and at every step; and for random finite inputs over the whole binary32 range,
                  denormals and zeros included.  Equality is allowed (+inf on both sides, say), less never.
soundness         thr >= |F64(q)| + E(q) at every point of those rays, the value the device may have computed at the previous
                  point being ANY binary32 number within E of the binary64 one (tests/test_anchor_cpu.py's model of F_a).
                  It follows from new >= old and the old proof; it is held directly all the same.
the anchored form as tests/test_anchor_cpu.py holds the old one: q on the start sphere, the anchor anywhere.
what it costs     new - old is at most 4e-6 (|ro|_1 + sqrt(3) |sc| - |q|_1), what the bound gives away, plus the reserves of the
                  constants and the roundings: 5e-5 of the term's own scale, and 5e-7 of the threshold (2^-22 from the factor on
                  the large term, 2^-24 for each of the roundings of thr_base, thr and the old thr).
non-finite        a non-finite sc, sd or f0 gives a threshold that is +inf or NaN; a non-finite d with a finite sc leaves it
                  finite but makes q non-finite, and the wave's mask (tests/wave_reach_model.py) then keeps every unit."""
import numpy as np
import pytest

import anchor_ref as A
import scene_f64
import scenes
import step_thr_ref as S
import wave_reach_model as M
from test_cull_tables_cpu import decode

F = np.float32
MAX_DIST = 100.0
MIN_DIST = 0.01
N_RAYS = 300
N_STEPS = 40


def cameras(oracle, centre):
    out = []
    for radius in (5.0, 50.0):
        _, pos, _, _ = oracle.orbit_uniforms((64.0, 64.0), target=tuple(centre), radius=radius, events=scenes.STILL_CAMERA_EVENTS)
        out.append(np.array(pos, dtype=F))
    return out


def device_value(f64, err, how):
    """a binary32 number within err of f64 (tests/test_anchor_cpu.py): |.| rounded towards zero so that it stays inside on the side
    that matters"""
    sd = {"rounded": f64, "F - E": f64 - err, "F + E": f64 + err, "|F| - E": np.sign(f64) * np.maximum(np.abs(f64) - err, 0.0)}[how]
    sd32 = sd.astype(F)
    up = np.abs(sd32.astype(np.float64)) > np.abs(sd)
    return np.where(up, np.nextafter(sd32, F(0.0)), sd32).astype(F)


def extra_allowed(ps, ro, sc, q, old):
    ro1 = np.abs(ro.astype(np.float64)).sum()
    sc1 = np.abs(sc.astype(np.float64))
    q1 = np.abs(q.astype(np.float64)).sum(axis=-1)
    scale = float(ps) + ro1 + 2.0 * sc1
    return 4.0e-6 * (ro1 + np.sqrt(3.0) * sc1 - q1) + 5.0e-5 * 4.0e-6 * scale + 5.0e-7 * old + 1.0e-29


@pytest.mark.parametrize("how", ["rounded", "F - E", "F + E", "|F| - E"])
@pytest.mark.parametrize("name", A.PAIR_PROGRAMS)
def test_marched_rays(oracle, name, how):
    cc, w, centre = A.program(oracle, name)
    scene_scale = decode(cc, w)["scene_scale"]
    rng = np.random.default_rng(2500 + A.PAIR_PROGRAMS.index(name))
    head, grow, n_pts = np.inf, 0.0, 0
    for ro in cameras(oracle, centre):
        ps = A.prune_scale(scene_scale, ro)
        c0 = S.step_thr_c0(ps, ro)
        f0 = F(scene_f64.map_scene(cc, w, MAX_DIST, ro[None])[0])
        assert MIN_DIST < f0 < MAX_DIST
        d = S.directions(ro, centre, rng, N_RAYS)
        sc = np.full(N_RAYS, F(0.0) + f0, dtype=F)
        # the hand-out: the camera's bound alone for even rays, the minimum with an anchor at ray 0's first point for odd ones
        q = S.point(ro, d, sc)
        a = q[:1]
        fa = scene_f64.map_scene(cc, w, MAX_DIST, a)
        aT = A.anchor_reach(a, device_value(fa, A.eval_error(ps, a), how), ps)
        cam = np.full(N_RAYS, S.old_thr_base(f0), dtype=F)
        tb_old = np.where(np.arange(N_RAYS) % 2 == 1, A.anchor_thr_base(cam, q, np.broadcast_to(a, q.shape), aT), cam).astype(F)
        assert np.any(tb_old < cam) or name == "degenerate"
        tb_new = S.handout_thr_base(tb_old, c0)
        live = np.ones(N_RAYS, dtype=bool)
        for step in range(N_STEPS):
            q = S.point(ro, d, sc)
            new, old = S.step_thr(tb_new, sc), A.step_threshold(tb_old, q, ps)
            assert np.all(new[live] >= old[live]), (name, step, int(np.argmin(new - old)))
            fq = scene_f64.map_scene(cc, w, MAX_DIST, q)
            err = A.eval_error(ps, q)
            need = np.abs(fq) + err
            k = int(np.argmin(np.where(live, new - need, np.inf)))
            assert np.all(new.astype(np.float64)[live] >= need[live]), "%s, camera %s, step %d, ray %d: thr %.9g < |F(q)| + E = %.9g" % (
                name, ro.tolist(), step, k, new[k], need[k])
            head = min(head, float(((new - need)[live] / float(ps)).min()))
            extra = new.astype(np.float64) - old.astype(np.float64)
            assert np.all(extra[live] <= extra_allowed(ps, ro, sc, q, old.astype(np.float64))[live]), (name, step)
            grow = max(grow, float((extra / old)[live].max()))
            n_pts += int(live.sum())
            sd = device_value(fq, err, how)
            live &= ~(sd < F(MIN_DIST)) & ~(sd > F(MAX_DIST))
            if not live.any():
                break
            tb_old, tb_new = S.old_thr_base(sd), S.step_thr_base(sd, c0)
            with np.errstate(all="ignore"):
                sc = np.where(live, (sc + sd).astype(F), sc).astype(F)
    print("%s, %s: %d points, smallest (thr - |F| - E) / prune_scale %.3g, largest (new - old) / old %.3g" % (name, how, n_pts, head, grow))
    assert n_pts > 4 * N_RAYS and head >= 0.0


def _magnitudes(rng, n):
    """binary32 magnitudes over the whole range: zeros, denormals, tiny, ordinary, huge"""
    x = (10.0 ** rng.uniform(-46.0, 30.0, n)).astype(F)
    x[rng.random(n) < 0.05] = F(0.0)
    return x


def test_new_is_at_least_old_for_random_finite_inputs():
    rng = np.random.default_rng(2510)
    n = 400000
    scale = _magnitudes(rng, n)
    ro = (_magnitudes(rng, 3 * n).reshape(n, 3) * rng.choice([-1.0, 1.0], (n, 3))).astype(F)
    d = np.asarray(S.R.unit(rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 0, (n, 3))), dtype=F)
    d[::9] = np.eye(3, dtype=F)[rng.integers(0, 3, len(d[::9]))]                # along an axis: |d|_1 = |d|_2
    d[1::9] = (np.sign(d[1::9]) + (d[1::9] == 0)) * F(np.sqrt(1.0 / 3.0))       # along a body diagonal: |d|_1 = sqrt(3) |d|_2
    assert np.all(np.linalg.norm(d.astype(np.float64), axis=1) <= 1.0 + 1.0e-6)
    sc = (_magnitudes(rng, n) * rng.choice([-1.0, 1.0], n)).astype(F)
    sd = (_magnitudes(rng, n) * rng.choice([-1.0, 1.0], n)).astype(F)
    # (scales of one another's size are where the roundings meet: tie half of the inputs to a common magnitude)
    tie = rng.random(n) < 0.5
    common = _magnitudes(rng, n)
    for arr in (scale, sc, sd):
        arr[tie] = (arr[tie] / np.maximum(np.abs(arr[tie]), F(1e-45)) * common[tie] * rng.uniform(0.1, 10.0, tie.sum())).astype(F)
    ro[tie] = (np.sign(ro[tie]) * common[tie, None] * rng.uniform(0.0, 10.0, (tie.sum(), 3))).astype(F)
    with np.errstate(all="ignore"):
        ps = (scale + A.l1(ro)).astype(F)
        c0 = (S.K_PRUNE_ABS_UP * (ps + A.l1(ro)).astype(F) + S.C0_FLOOR).astype(F)
        q = (ro + (d * sc[:, None]).astype(F)).astype(F)
        ok = np.isfinite(ps) & np.isfinite(q).all(axis=1)
        assert ok.mean() > 0.9
        # a step
        new = S.step_thr(S.step_thr_base(sd, c0), sc)
        old = (S.old_thr_base(sd) + A.K_PRUNE_ABS * (ps + A.l1(q)).astype(F)).astype(F)
        k = int(np.argmin(np.where(ok, new - old, np.inf)))
        assert np.all(new[ok] >= old[ok]), (ro[k].tolist(), d[k].tolist(), float(sc[k]), float(sd[k]), float(scale[k]), float(new[k]), float(old[k]))
        # the hand-out: T any non-negative number, +inf included
        T = np.abs(sd)
        T[::11] = F(np.inf)
        new = S.step_thr(S.handout_thr_base(T, c0), sc)
        old = (T + A.K_PRUNE_ABS * (ps + A.l1(q)).astype(F)).astype(F)
        assert np.all(new[ok] >= old[ok])
        assert np.all(np.isinf(new[ok][::11][np.isinf(T[ok][::11])]))


def test_the_anchored_form_bounds_the_value_on_the_start_sphere(oracle):
    for name in A.PAIR_PROGRAMS:
        cc, w, centre = A.program(oracle, name)
        scene_scale = decode(cc, w)["scene_scale"]
        rng = np.random.default_rng(2520 + A.PAIR_PROGRAMS.index(name))
        for ro in cameras(oracle, centre):
            ps = A.prune_scale(scene_scale, ro)
            c0 = S.step_thr_c0(ps, ro)
            f0 = F(scene_f64.map_scene(cc, w, MAX_DIST, ro[None])[0])
            n = 1500
            sc = np.full(n, F(0.0) + f0, dtype=F)
            q = S.point(ro, S.directions(ro, centre, rng, n), sc)
            a = A.pairs(ro, centre, abs(float(f0)), rng, n)[:, 0]                 # on the start sphere and anywhere
            fa, fq = scene_f64.map_scene(cc, w, MAX_DIST, a), scene_f64.map_scene(cc, w, MAX_DIST, q)
            need = np.abs(fq) + A.eval_error(ps, q)
            for how in ("rounded", "F - E", "F + E", "|F| - E"):
                aT = A.anchor_reach(a, device_value(fa, A.eval_error(ps, a), how), ps)
                tb = A.anchor_thr_base(S.old_thr_base(f0), q, a, aT)
                new = S.step_thr(S.handout_thr_base(tb, c0), sc)
                assert np.all(new >= A.step_threshold(tb, q, ps)), (name, how)
                k = int(np.argmin(new - need))
                assert np.all(new.astype(np.float64) >= need), "%s, %s: a %s q %s: thr %.9g < |F(q)| + E = %.9g" % (
                    name, how, a[k].tolist(), q[k].tolist(), new[k], need[k])


def test_non_finite_inputs_give_a_threshold_under_which_nothing_is_skipped(oracle):
    cc, w, centre = A.program(oracle, "g32")
    dec = decode(cc, w)
    ro = cameras(oracle, centre)[0]
    ps = A.prune_scale(dec["scene_scale"], ro)
    c0 = S.step_thr_c0(ps, ro)
    assert np.isfinite(c0) and c0 > 0
    bad = np.array([np.nan, np.inf, -np.inf], dtype=F)
    fine = np.array([0.0, 1.0e-3, 0.7, 40.0], dtype=F)
    for tb in (S.step_thr_base(fine, c0), S.handout_thr_base(S.old_thr_base(fine), c0), np.full(4, np.inf, dtype=F)):
        for x in bad:                                               # a non-finite sc
            thr = S.step_thr(tb, np.full(4, x, dtype=F))
            assert not np.any(np.isfinite(thr)) and not np.any(thr == -np.inf)
    for x in bad:                                                   # a non-finite sd, a non-finite f0
        for tb in (S.step_thr_base(np.full(4, x, dtype=F), c0), S.handout_thr_base(S.old_thr_base(np.full(4, x, dtype=F)), c0)):
            assert np.all(np.isnan(tb)) if np.isnan(x) else np.all(tb == np.inf)
            thr = S.step_thr(tb, fine)
            assert not np.any(np.isfinite(thr)) and not np.any(thr == -np.inf)
    assert np.all(S.handout_thr_base(np.full(4, np.inf, dtype=F), c0) == np.inf)          # a ray that does not take the shared step
    # a non-finite d with a finite sc: thr stays finite, q does not, and the wave's mask keeps every unit
    units_p = np.array([u["p"][:4] for u in dec["units"]])
    valid = np.uint64((1 << len(units_p)) - 1)
    rng = np.random.default_rng(2530)
    n_waves = 96
    # (a wave's rays come from one tile and march in step: neighbouring directions, nearly the same distance)
    d0 = S.directions(ro, centre, rng, n_waves).astype(np.float64)
    d = np.stack([S.R.unit(d0[wv][None] + rng.normal(size=(64, 3)) * 0.004) for wv in range(n_waves)]).astype(F)
    sc = (rng.uniform(1.0, 4.0, (n_waves, 1)) + rng.uniform(0.0, 0.01, (n_waves, 64))).astype(F)
    sc[::4] = F(0.0)                                                 # inf * 0 = NaN
    thr = S.step_thr(S.step_thr_base(rng.uniform(0.0, 0.05, (n_waves, 64)).astype(F), c0), sc)
    live = rng.integers(1, 2 ** 63, n_waves, dtype=np.uint64) | np.uint64(1)
    clean, _ = M.lattice_masks(units_p, S.point(ro, d, sc), thr, live)
    assert (clean != valid).sum() > n_waves // 2                    # (there is something to lose)
    lanes = M.live_lanes(live)
    for wv in range(n_waves):
        lane = int(rng.choice(np.flatnonzero(lanes[wv])))
        d[wv, lane, int(rng.integers(3))] = bad[wv % 3]
    q = S.point(ro, d, sc)
    assert np.all(np.isfinite(thr)) and np.all((~np.isfinite(q)).any(axis=2).any(axis=1))
    masks, _ = M.lattice_masks(units_p, q, thr, live)
    assert np.all(masks == valid)
