"""The L1 reach of wave_cull_lattice without a GPU: tests/wave_reach_model.py restates the rule in binary32, operation by operation
(tests/test_gpu_wave_reach.py holds the kernel to that restatement, mask for mask), and whatever the model skips must be far in
binary64: |p_l - c| - R > thr_l at every live lane.  About 10^4 waves: random clouds at the origin and 1e3 and 1e5 from it, reaches
from 1e-6 to 10, denormal offsets, lanes that coincide, and the waves of the GPU test, whose reach ends within 1e-5 of a unit."""
import numpy as np
import pytest

import wave_reach_model as M
from div_ref import fma as fma_bits

F = np.float32


def test_fma32_is_the_correctly_rounded_fused_multiply_add():
    """Against the integer arithmetic of tests/div_ref.py, on operands that cancel, that tie and that differ by many binades."""
    rng = np.random.default_rng(140)
    a = (rng.uniform(1, 2, 4000) * 2.0 ** rng.integers(-30, 30, 4000)).astype(F)
    b = (rng.uniform(1, 2, 4000) * 2.0 ** rng.integers(-30, 30, 4000)).astype(F) * rng.choice([-1, 1], 4000).astype(F)
    c = np.empty(4000, dtype=F)
    c[:1000] = (rng.uniform(1, 2, 1000) * 2.0 ** rng.integers(-60, 60, 1000)).astype(F)
    c[1000:2000] = -(a[1000:2000] * b[1000:2000]) * (1 + rng.integers(-3, 4, 1000) * 2.0 ** -23).astype(F)     # near cancellation
    c[2000:3000] = (a[2000:3000].astype(np.float64) * b[2000:3000] * 2.0 ** rng.integers(-26, -22, 1000)).astype(F)   # c near half an ulp
    c[3000:] = (a[3000:].astype(np.float64) * b[3000:] * 2.0 ** rng.integers(22, 27, 1000)).astype(F)             # the product near half an ulp
    got = M.fma32(a, b, c).view(np.uint32)
    want = np.array([fma_bits(int(x), int(y), int(z)) for x, y, z in zip(a.view(np.uint32), b.view(np.uint32), c.view(np.uint32))], dtype=np.uint32)
    assert np.array_equal(got, want)
    assert M.fma32(F(3), F(1.00001), F(np.inf)) == np.inf and np.isnan(M.fma32(F(np.nan), F(1), F(0)))


def _random_units(rng, centre, n):
    p = np.zeros((n, 4))
    p[:, :3] = centre + rng.uniform(-3, 3, (n, 3))
    p[:, 3] = rng.choice([0.0, 1e-4, 0.3, 0.9, 2.0], n) * rng.uniform(0.5, 1.0, n)
    return p.astype(F).astype(np.float64)


def _cloud_waves(units_p, centre, rng, n_waves):
    """Random clouds: Gaussian, or on a line, or all lanes in one point; offsets down to the denormals far from nowhere."""
    pos = np.zeros((n_waves, 64, 3), dtype=F)
    thr = np.zeros((n_waves, 64), dtype=F)
    live = np.zeros(n_waves, dtype=np.uint64)
    for wv in range(n_waves):
        p0 = centre + rng.uniform(-4, 4, 3)
        spread = 10.0 ** rng.uniform(-6, 1)
        kind = wv % 4
        if kind == 0:
            p = p0 + rng.normal(size=(64, 3)) * spread
        elif kind == 1:
            p = p0 + rng.normal(size=3) * rng.uniform(-1, 1, (64, 1)) * spread
        elif kind == 2:
            p = np.repeat(p0[None, :], 64, axis=0)
        else:
            p = rng.normal(size=(64, 3)) * 10.0 ** rng.uniform(-44, -36)      # around the origin, among the denormals
        pos[wv] = p.astype(F)
        thr[wv] = (rng.uniform(0, 1, 64) * float(rng.choice([0.0, 1e-40, 1e-3, 0.1, 1.0, 3.0]))).astype(F)
        live[wv] = np.uint64(0xFFFFFFFFFFFFFFFF) if wv % 3 == 0 else (rng.integers(1, 2 ** 63, dtype=np.uint64) | np.uint64(1 << int(rng.integers(64))))
    return pos, thr, live


@pytest.mark.parametrize("off", [0.0, 1.0e3, 1.0e5])
def test_what_the_model_skips_is_far_in_binary64(off):
    rng = np.random.default_rng(141 + int(off))
    centre = np.array([off, -off, off])
    counts = {"skipped": 0, "kept": 0, "sharp waves": 0, "must skip": 0}
    n_waves = 0
    for _ in range(6):
        units_p = _random_units(rng, centre, int(rng.integers(2, 33)))
        for maker in (lambda: _cloud_waves(units_p, centre, rng, 300), lambda: M.reach_waves(units_p, rng, 300)):
            pos, thr, live = maker()
            masks, _ = M.lattice_masks(units_p, pos, thr, live)
            M.check_masks("units around %g" % off, units_p, pos, thr, live, masks, counts)
            n_waves += len(pos)
    print("model at %g: %d waves, %s" % (off, n_waves, counts))
    assert n_waves == 3600
    assert counts["skipped"] > 10000 and counts["kept"] > 5000, counts            # (of about 60 000 decisions)
    assert counts["must skip"] > 5000, counts


def test_special_lanes_in_the_model():
    rng = np.random.default_rng(142)
    units_p = _random_units(rng, np.zeros(3), 12)
    pos, thr, live = M.reach_waves(units_p, rng, 64)
    masks, _ = M.lattice_masks(units_p, pos, thr, live)
    assert (masks != np.uint64(0xFFF)).any()
    lv = M.live_lanes(live)
    for what in ("thr nan", "thr inf", "pos nan", "pos inf", "pos -inf"):
        for lane_of in (lambda w: int(np.argmax(lv[w])), lambda w: int(rng.choice(np.flatnonzero(lv[w])))):
            p, t = pos.copy(), thr.copy()
            for w in range(64):
                lane = lane_of(w)
                if what.startswith("thr"):
                    t[w, lane] = np.nan if what == "thr nan" else np.inf
                else:
                    p[w, lane, int(rng.integers(3))] = {"pos nan": np.nan, "pos inf": np.inf, "pos -inf": -np.inf}[what]
            assert np.all(M.lattice_masks(units_p, p, t, live)[0] == np.uint64(0xFFF)), what
    p, t = pos.copy(), thr.copy()
    p[~lv] = rng.choice([np.nan, np.inf, -np.inf, 1e30], size=p.shape).astype(F)[~lv]
    t[~lv] = rng.choice([np.nan, np.inf, 1e30], size=t.shape).astype(F)[~lv]
    assert np.array_equal(M.lattice_masks(units_p, p, t, live)[0], masks)
    # a single live lane: S is its own threshold times the two factors that still apply
    one = np.uint64(1) << rng.integers(0, 64, 64).astype(np.uint64)
    only = M.live_lanes(one)
    p = np.where(only[:, :, None], pos, F(np.nan))
    _, S = M.lattice_masks(units_p, p, thr, one)
    own = thr[only]
    assert np.array_equal(S, M.fma32(F(0), M.K_REACH, own) * M.K_S)
