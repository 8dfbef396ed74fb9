"""wave_cull_lattice with its reach in the L1 norm ("Wave-level culling"), through rm_selftest_cull_waves as
tests/test_gpu_cull_bounds.py drives it: a few hundred 64-lane waves per program, the smallest shape the function has.

soundness   where the two norms differ most: live lanes spread from p* along the body diagonals (L1 = sqrt(3) L2) and along the axes
            (L1 = L2) over 1e-4 .. 10, thresholds so that the wave's L2 reach and its L1 reach each end within +-1e-5 and +-1e-3 (and
            +-2e-4, twice the sharpness margin) of a unit's outer sphere, in half of the waves with the deciding lane straight between
            p* and the unit, where the triangle inequality is tight (tests/wave_reach_model.py reach_waves).  For every skipped unit the
            leaf's value is above the lane's threshold at every live lane, in binary64 and in the oracle's binary32.
sharpness   the rule must not pass by skipping nothing: with S1 = max over live lanes (|p_l - p*|_1 + thr_l) in binary64 from the
            binary32 inputs, every unit with a finite bound and |p* - c| - R > S1 (1 + 1e-4) is skipped.  The rule's own slack
            factors, 1.00001 on the reach, 1.000005 on the maximum and 1.000004 on the squares, multiply to 1 + 1.70e-5
            (wave_reach_model.RULE_SLACK); the margin 1e-4 is 5.9 times that.  The comparison is made in binary32 on |p* - c| and
            S + R, so it resolves 2.4e-6 of |p* - c|, not of S1: the claim is made for the waves whose S1 is at least 0.04 of the
            farthest unit's distance (derivation beside wave_reach_model.SHARP_MIN_REACH), which most waves here are.
            At least a third of the (wave, unit) decisions fall on each side.
the model   every mask equals the binary32 restatement of the rule that tests/test_wave_reach_cpu.py checks without a GPU.
special lanes   a NaN or +inf threshold, or a NaN or infinite coordinate, in one live lane gives the full mask; garbage in dead lanes
            changes nothing; a wave with a single live lane has reach = its own threshold."""
import math

import numpy as np
import pytest

import cull_ref as R
import scene_f64  # noqa: F401  (through _leaf_values)
import scenes
import wave_reach_model as M
from test_cull_tables_cpu import decode
from test_gpu_cull_bounds import _leaf_values, _shift, probe_waves, set_case

pytestmark = pytest.mark.gpu

F = np.float32
TWO_LEAVES = [(0, [0.0, 0.0, 0.0, 0.5]), (1, [1.2, 0.1, 0.0, 0.4, 0.3, 0.5]), (100, [])]
FAR = (1e3, -1e3, 1e3)
N_WAVES = 256


@pytest.fixture(scope="module")
def res():
    from ray_marching_amd import renderer
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(8192)
    yield r
    r.close()


def reach_programs(oracle):
    cc, w = oracle.serialize(*{**scenes.SCENES, **scenes.EXT_SCENES}["g32"]())
    return [("g32", cc, np.asarray(w, dtype=np.uint32), np.zeros(3)),
            ("two leaves", *R.words_of(*TWO_LEAVES), np.zeros(3)),
            ("two leaves at 1e3", *R.words_of(*_shift(TWO_LEAVES, FAR)), np.array(FAR))]


def units_of(d):
    return np.array([u["p"][:4] for u in d["units"]])


@pytest.fixture(scope="module")
def cases(res, oracle):
    """[(name, decoded program, units, pos, thr, live, masks)]: the probe runs once per program, every test reads its masks"""
    out = []
    rng = np.random.default_rng(143)
    for name, cc, w, centre in reach_programs(oracle):
        d = decode(cc, w)
        assert d["unit_mode"] == 1, name
        set_case(res, cc, w, 0.01)
        units_p = units_of(d)
        pos, thr, live = M.reach_waves(units_p, rng, N_WAVES)
        ro = (centre + [0.0, 0.0, 5.0]).astype(F)
        masks = probe_waves(res, ro, pos, thr, live)
        for a in (pos, thr, live, masks):
            a.setflags(write=False)
        out.append((name, cc, w, ro, d, units_p, pos, thr, live, masks))
    return out


def test_skipped_units_are_far_and_far_units_are_skipped(cases):
    total = {"skipped": 0, "kept": 0, "sharp waves": 0, "must skip": 0}
    for name, cc, w, ro, d, units_p, pos, thr, live, masks in cases:
        counts = {"skipped": 0, "kept": 0, "sharp waves": 0, "must skip": 0}
        M.check_masks(name, units_p, pos, thr, live, masks, counts)
        print("%s: %s" % (name, counts))
        assert counts["sharp waves"] * 2 >= N_WAVES, (name, counts)
        for k in counts:
            total[k] += counts[k]
    n = total["skipped"] + total["kept"]
    assert total["skipped"] * 3 >= n and total["kept"] * 3 >= n, total
    assert total["must skip"] * 3 >= n, total


def test_skipped_leaves_are_above_every_live_lanes_threshold(cases):
    """The leaf itself, not its bounding sphere: scene_f64 and the oracle's binary32 arithmetic."""
    head = math.inf
    for name, cc, w, ro, d, units_p, pos, thr, live, masks in cases:
        lv = M.live_lanes(live)
        scale = d["scene_scale"] + np.abs(ro).sum()
        for ui, u in enumerate(d["units"]):
            gone = ((masks >> np.uint64(ui)) & np.uint64(1)) == 0
            if not gone.any():
                continue
            sel = lv[gone]
            pts, t = pos[gone][sel], thr[gone][sel].astype(np.float64)
            for label, v in zip(("binary64", "binary32"), _leaf_values(d, u, pts)):
                k = int(np.argmin(v - t))
                assert np.all(v > t), "%s unit %d: skipped, but its %s value %.9g at %s is not above the lane's threshold %.9g" % (
                    name, ui, label, v[k], pts[k].tolist(), t[k])
                head = min(head, float((v - t).min() / scale))
    print("smallest (value - thr) / scale of a skipped leaf: %.3g" % head)


def test_masks_are_the_models(cases):
    for name, cc, w, ro, d, units_p, pos, thr, live, masks in cases:
        want, _ = M.lattice_masks(units_p, pos, thr, live)
        diff = np.flatnonzero(want != masks)
        assert len(diff) == 0, "%s: wave %d: the kernel's mask %x, the model's %x" % (name, diff[0], int(masks[diff[0]]), int(want[diff[0]]))


def test_special_lanes(res, cases):
    rng = np.random.default_rng(144)
    for name, cc, w, ro, d, units_p, pos, thr, live, masks in cases:
        set_case(res, cc, w, 0.01)
        valid = np.uint64((1 << len(units_p)) - 1)
        assert (masks != valid).sum() > N_WAVES // 4, name           # (there is something to lose)
        lv = M.live_lanes(live)
        # one live lane -- the first, which is p*, in even waves, any in odd ones -- with a threshold or a coordinate that is no number
        for what in ("thr nan", "thr inf", "pos nan", "pos inf", "pos -inf"):
            p, t = pos.copy(), thr.copy()
            for wv in range(N_WAVES):
                lane = int(np.argmax(lv[wv])) if wv % 2 == 0 else int(rng.choice(np.flatnonzero(lv[wv])))
                if what.startswith("thr"):
                    t[wv, lane] = np.nan if what == "thr nan" else np.inf
                else:
                    p[wv, lane, int(rng.integers(3))] = {"pos nan": np.nan, "pos inf": np.inf, "pos -inf": -np.inf}[what]
            assert np.all(probe_waves(res, ro, p, t, live) == valid), (name, what)
        # garbage in the dead lanes
        p, t = pos.copy(), thr.copy()
        p[~lv] = rng.choice([np.nan, np.inf, -np.inf, 1e30], size=p.shape).astype(F)[~lv]
        t[~lv] = rng.choice([np.nan, np.inf, 1e30], size=t.shape).astype(F)[~lv]
        assert np.array_equal(probe_waves(res, ro, p, t, live), masks), name
        # a single live lane, the others dead and holding garbage: S1 is its own threshold, the same two claims hold with it
        lane = rng.integers(0, 64, N_WAVES)
        one = np.uint64(1) << lane.astype(np.uint64)
        only = M.live_lanes(one)
        p = np.where(only[:, :, None], pos, p)
        p[~only & lv] = F(np.nan)
        t = np.where(only, (np.abs(thr) + F(0.05)) * F(rng.choice([1.0, 8.0, 40.0])), F(np.nan)).astype(F)
        got = probe_waves(res, ro, p, t, one)
        star, s1, s2 = M.reaches(p, t, one)
        assert np.array_equal(s1, t[only].astype(np.float64)) and np.array_equal(s1, s2)
        counts = {"skipped": 0, "kept": 0, "sharp waves": 0, "must skip": 0}
        M.check_masks(name + ", one live lane", units_p, p, t, one, got, counts)
        assert np.array_equal(got, M.lattice_masks(units_p, p, t, one)[0]), name
        assert counts["must skip"] > 0 and counts["kept"] > 0, (name, counts)
