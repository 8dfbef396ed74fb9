"""The inputs of tests/test_gpu_query_fuzz.py are what tests/fuzz_programs.py says they are -- checked on the references alone
(the oracles, the host decoder, tests/gbuffer_ref.py), so that the GPU comparison cannot pass on programs that exercise nothing:
every seed of every class is a valid program of its class, the general programs nest transforms and spill values, the
constructed tie points are exact ties of the two operands, both oracles agree on the material there, every frame shows
surface, floor and sky, and the rays end in every way a march can end."""
import numpy as np
import pytest

import fuzz_programs as FP
import gbuffer_ref
import light_ref
import mesh_ref
from oracle import rm_oracle_np as onp
from test_gpu_query import march_replay
from ray_marching_amd import renderer

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- the random programs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", FP.CLASSES)
def test_every_seed_gives_a_valid_program_of_its_class(oracle, cls):
    cases = [FP.case(oracle, cls, seed) for seed in FP.SEEDS]          # raises if a seed gives nothing: no seed is left out
    for c in cases:
        assert oracle.validate(c.cc, c.words)[0] == 0 and renderer.validate_program(c.cc, c.words)[0] == 0, FP.describe(c)
        assert c.info["is_chain"] == (1 if cls == "chain" else 0), FP.describe(c)
        ops = set(FP.opcodes(c.cc, c.words))
        if cls == "general":
            assert not ops <= set(FP.CORE), FP.describe(c)             # an extension node: neither the chain nor the tree loop
        else:
            assert ops <= set(FP.CORE), FP.describe(c)
        assert c.limits[0] in (0.01, 0.2) and c.limits[1] in (100.0, 6.0) and c.limits[2] in (24, 64)
        assert c.table.shape == (8, 3)
    # the same seed names the same case
    FP._cases.pop((cls, FP.SEEDS[0]))
    again = FP.case(oracle, cls, FP.SEEDS[0])
    assert again.cc == cases[0].cc and np.array_equal(again.words, cases[0].words) and again.events == cases[0].events
    assert again.limits == cases[0].limits and np.array_equal(again.table, cases[0].table)
    if cls == "general":
        n = len(cases)
        assert 3 * sum(c.info["has_xforms"] == 1 for c in cases) >= n
        assert 3 * sum(c.info["spill_depth"] >= 3 for c in cases) >= n
        assert any(300 in FP.opcodes(c.cc, c.words) for c in cases)   # tags: the walk's material byte
    if cls == "tree":
        assert any(c.info["spill_depth"] >= 2 for c in cases)         # not left-deep


@pytest.mark.parametrize("cls", FP.CLASSES)
def test_every_frame_shows_surface_floor_and_sky(oracle, cls):
    """The reference G-buffer of every seed at the test's size; over the class, pixels whose samples disagree."""
    partial = several = 0
    for seed in FP.SEEDS:
        c = FP.case(oracle, cls, seed)
        want, records = gbuffer_ref.render(c.ud, c.limits, c.cc, c.words, FP.W, FP.H, detail=True)
        kinds = set(int(k) for r in records for k in np.unique(r["kind"]))
        assert kinds == {0, 1, 2}, FP.describe(c)
        assert want["surface_mask"].any() and want["floor_mask"].any(), FP.describe(c)
        assert ((want["surface_mask"] | want["floor_mask"]) != 0xFFFF).any(), FP.describe(c)      # sky
        partial += int(((want["surface_mask"] != 0) & (want["surface_mask"] != 0xFFFF)).sum())
        leaves = np.stack([np.where(r["kind"] == 1, r["leaf"], gbuffer_ref.RM_NO_ID) for r in records]).astype(np.int64)
        lo = np.where(leaves == gbuffer_ref.RM_NO_ID, 1 << 40, leaves).min(axis=0)
        hi = np.where(leaves == gbuffer_ref.RM_NO_ID, -1, leaves).max(axis=0)
        several += int(((hi >= 0) & (lo != hi)).sum())
    print("%s: pixels with a partial surface mask %d, with several leaves %d" % (cls, partial, several))
    assert partial > 0 and several > 0


@pytest.mark.parametrize("cls", FP.CLASSES)
def test_the_rays_end_in_every_way(oracle, cls):
    kinds, ran_out = set(), 0
    for seed in FP.SEEDS:
        c = FP.case(oracle, cls, seed)
        kind, steps, t, pos = march_replay(c.cc, c.words, c.limits, FP.rays_of(c))
        kinds |= set(int(k) for k in np.unique(kind))
        ran_out += int(((kind != 1) & (steps == c.limits[2])).sum())
    assert kinds == {0, 1, 2} and ran_out > 0


# ---- the constructed programs ----------------------------------------------------------------------------------------------------
def operands_at(c, p):
    with np.errstate(all="ignore"):
        a = onp.map_scene(c.a[0], c.a[1], F(c.limits[1]), p[:, 0], p[:, 1], p[:, 2])
        b = onp.map_scene(c.b[0], c.b[1], F(c.limits[1]), p[:, 0], p[:, 1], p[:, 2])
    return a, b


def test_tie_points_are_exact_ties(oracle):
    cases = FP.tie_cases(oracle)
    assert len(cases) == 35 and len(set(c.name for c in cases)) == 35          # (+ nan_case: the GPU test's N_TIES)
    for c in cases:
        assert oracle.validate(c.cc, c.words)[0] == 0 and renderer.validate_program(c.cc, c.words)[0] == 0, c.name
        sub = c.name.startswith("subtraction")
        a, b = operands_at(c, c.ties)
        assert len(c.ties) >= 2 and np.all(np.isfinite(a)), c.name
        assert np.array_equal(bits(a), bits(b)), c.name                 # bitwise equal operands ...
        with np.errstate(all="ignore"):
            assert np.all((a == -b) if sub else (a == b)), c.name       # ... that tie in the comparison the operator makes
            p = FP.tie_point_set(c)
            a, b = operands_at(c, p)
            tie = (a == -b) if sub else (a == b)
            assert tie.any() and (~tie).any(), c.name                   # (no tie: other points, or NaN operands)
            if len(c.others):
                a, b = operands_at(c, c.others)
                assert not np.any((a == -b) if sub else (a == b)), c.name
        assert np.isnan(p).any() and np.isinf(p).any() and np.signbit(p[p == 0]).any(), c.name
        # the two operands are distinct command ranges of the program, each a tagged primitive
        assert c.first[1] == 2 and c.second[1] == 2 and c.second[0] == c.first[0] + 2, (c.name, c.first, c.second)
    # the record loop each names (the GPU test asserts it): a tag is an extension node, so none takes the tree loop; two tagged
    # leaves under Union / Subtraction are a chain without their tags -- the chain loop under the walk's LDS layout
    assert all(c.loop == ("chain" if c.info["is_chain"] else "general") for c in cases)
    assert sorted(c.name for c in cases if c.loop == "chain") == [
        "subtraction of duplicates, plain", "union of duplicates, plain", "union of mirror spheres, plain"]


def test_the_first_operand_wins_a_tie_in_both_oracles(oracle):
    """What the written contract says (Material): ties and NaN keep a's tag; Subtraction of duplicates
    carries b's inside and a's outside."""
    by_name = {c.name: c for c in FP.tie_cases(oracle)}
    for name, c in by_name.items():
        if name.endswith("chain") or name.endswith("scale"):
            continue                                                    # (the other operands of the root may win there)
        p = c.ties
        with np.errstate(all="ignore"):
            _, m = onp.map_scene(c.cc, c.words, F(c.limits[1]), p[:, 0], p[:, 1], p[:, 2], want_material=True)
        assert np.all(m == 1), name
    c = by_name["subtraction of duplicates, plain"]
    for p, want in (((0.25, 0.0, 0.0), 2), ((0.25, 0.5, 0.0), 2), ((2.0, 0.0, 0.0), 1), ((1.0, 0.0, 0.0), 1)):
        assert oracle.map_scene_material(c.cc, c.words, np.array(p, F), c.limits) == want, p


def test_both_oracles_agree_on_the_material_at_every_constructed_point(oracle):
    nan = FP.nan_case(oracle)
    assert oracle.validate(nan.cc, nan.words)[0] == 0 and renderer.validate_program(nan.cc, nan.words)[0] == 0
    for c in FP.tie_cases(oracle) + [nan]:
        p = FP.tie_point_set(c)
        if c is not nan:
            p = np.concatenate([p[:len(c.ties) + len(c.others)], p[-400:]])       # the exact points and the tail of the mix
        with np.errstate(all="ignore"):
            d, m = onp.map_scene(c.cc, c.words, F(c.limits[1]), p[:, 0], p[:, 1], p[:, 2], want_material=True)
        for i in range(len(p)):
            assert oracle.map_scene_material(c.cc, c.words, p[i], c.limits) == int(m[i]), (c.name, p[i])
            dc = F(oracle.map_scene(c.cc, c.words, p[i], c.limits))
            assert bits(dc) == bits(d[i]) or (np.isnan(dc) and np.isnan(d[i])), (c.name, p[i])
    # the Scale by 0 gives what it is there for: at finite points the first Union's a is NaN, so the distance is the healthy
    # b's (NaN loses a minimum) under a's tag (b < NaN is false) -- and elsewhere other operands decide
    finite = np.all(np.isfinite(p), axis=1)
    assert np.all(np.isfinite(d[finite])) and 4 in m[finite] and len(np.unique(m[finite])) >= 2


def test_the_shadow_threshold_case_steps_at_exactly_min_dist(oracle):
    c = FP.shadow_threshold_case(oracle)
    assert oracle.validate(c.cc, c.words)[0] == 0 and c.info["is_chain"] == 1
    py, px = np.meshgrid(np.arange(FP.H, dtype=np.uint32), np.arange(FP.W, dtype=np.uint32), indexing="ij")
    n_exact = 0
    for s in range(16):
        r = gbuffer_ref.per_sample(px.ravel(), py.ravel(), s, c.ud, c.limits, c.cc, c.words, FP.W, FP.H)
        assert not (r["kind"] == 1).any()                      # one step: no primary ray reaches the box
        f = r["hit"][r["kind"] == 2, 1:4]
        with np.errstate(all="ignore"):
            h = onp.map_scene(c.cc, c.words, F(c.limits[1]), f[:, 0], f[:, 1], f[:, 2])
        n_exact += int((h == F(c.limits[0])).sum())
        assert not (h < F(c.limits[0])).any()
    assert n_exact > 100, n_exact
    # ... and those points are lit: had the step counted as a hit, their pixels would be darker
    p = light_ref.params(**c.light)
    lit = light_ref.render(c.ud, c.limits, c.cc, c.words, FP.W, FP.H, light=p)[0]
    unlit = light_ref.render(c.ud, c.limits, c.cc, c.words, FP.W, FP.H, light=light_ref.params(**light_ref.IDENTITY))[0]
    assert np.array_equal(lit, unlit)                           # nothing shadows this floor


@pytest.mark.parametrize("cls", FP.CLASSES)
def test_the_lattices_cut_the_surface(oracle, cls):
    """The 24^3 lattice of the GPU test's mesh extraction: at least half the seeds of a class give triangles."""
    origin, step, shape = (-3.0,) * 3, (F(6.0) / F(23),) * 3, (24, 24, 24)
    p = mesh_ref.lattice_points(origin, step, shape)
    with_triangles = 0
    for seed in FP.SEEDS:
        c = FP.case(oracle, cls, seed)
        with np.errstate(all="ignore"):
            d = onp.map_scene(c.cc, c.words, F(c.limits[1]), p[:, 0], p[:, 1], p[:, 2])
        with_triangles += len(mesh_ref.extract(np.asarray(d, F).reshape(24, 24, 24), origin, step, 0.0)[1]) > 0
    assert 2 * with_triangles >= len(FP.SEEDS), with_triangles
