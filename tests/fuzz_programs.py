"""Inputs of the query fuzz (tests/test_query_fuzz_cpu.py, tests/test_gpu_query_fuzz.py): seeded random CSG programs, one
generator per record loop of the interpreter ("The interpreter's record loops": general, tree, chain),
and constructed programs whose operands tie exactly or are NaN / inf.  TEST INFRASTRUCTURE; a plain module without fixtures.

A (class, seed) pair always names the same case: the program, its limits, its material table and its camera all come from
one generator seeded with (class, seed).  Inside the seed the generator redraws until
  - the oracle and the product validator accept the program,
  - the program has the class it is for (rm_program_info's is_chain and the opcodes it uses), and
  - one of up to eight cameras shows surface, floor and sky in sample 5 of the 21 x 13 frame (the reference's march),
so no seed is ever left out of a test.  tests/test_query_fuzz_cpu.py checks what is promised here, on the references alone."""
import math
import os
import types

import numpy as np

import gbuffer_ref
import scenes
from test_gpu_cull_differential import random_leaf
from test_gpu_fuzz import random_tree
from test_gpu_query import commands, sample_points, sample_rays
from ray_marching_amd import renderer

F = np.float32
CLASSES = ("general", "tree", "chain")
W, H = 21, 13                     # odd in both directions: edge 2 x 2 blocks and an 8 x 8 tile with idle lanes
CORE = (0, 1, 100, 101)           # sphere, box, Union, Subtraction: what the chain and the tree loop run
_SALT = {"general": 41000, "tree": 42000, "chain": 43000}
FIRST_SEED = int(os.environ.get("RM_QUERY_FUZZ_FIRST_SEED", "0"))
SEEDS = range(FIRST_SEED, FIRST_SEED + int(os.environ.get("RM_QUERY_FUZZ_SEEDS", "8")))
STILL = [(1, 35.0, -25.0)]


def opcodes(cc, words):
    return [op for _, op, _ in commands(words, cc)]


def uniforms_dict(u):
    return {"viewport_extent": list(u.viewport_extent), "inv_proj": list(u.inv_proj), "inv_view": list(u.inv_view)}


# ---- the three generators ------------------------------------------------------------------------------------------------------
def _general(rng, t):
    return random_tree(rng, t, int(rng.integers(4, 7)), allow_plane=bool(rng.random() < 0.3), tags=True)


def _tree_node(rng, t, depth, spread):
    if depth == 0 or rng.random() < 0.2:
        return random_leaf(rng, t, spread)
    a = _tree_node(rng, t, depth - 1, spread)
    b = _tree_node(rng, t, depth - 1, spread)
    return t.op(scenes.UNION if rng.random() < 0.65 else scenes.SUBTRACTION, a, b)


def _tree(rng, t):
    return _tree_node(rng, t, int(rng.integers(2, 6)), float(rng.choice([1.0, 1.8])))


def _chain(rng, t):
    spread = float(rng.choice([1.0, 1.8]))
    acc = random_leaf(rng, t, spread)
    for _ in range(int(rng.integers(1, 16))):
        acc = t.op(scenes.UNION if rng.random() < 0.65 else scenes.SUBTRACTION, acc, random_leaf(rng, t, spread))
    return acc


_BUILD = {"general": _general, "tree": _tree, "chain": _chain}


def has_class(cls, cc, words, seed=None):
    """The class by the decoder's facts: a chain is what rm_program_info calls one; a tree is any other program of spheres and
    boxes under Union / Subtraction; everything else takes the general loop.  With a seed, also what the general class
    promises about depth whatever the seed range: even seeds spill at least 3 values, odd seeds have a transform."""
    info = renderer.program_info(cc, words)
    core = set(opcodes(cc, words)) <= set(CORE)
    if cls == "chain":
        return info["is_chain"] == 1 and core
    if cls == "tree":
        return info["is_chain"] == 0 and core
    prims = sum(op in (0, 1, 2, 10) for op in opcodes(cc, words))
    if seed is not None and (info["spill_depth"] < 3 if seed % 2 == 0 else info["has_xforms"] == 0):
        return False
    return info["is_chain"] == 0 and not core and prims >= 4      # (a general program of fewer leaves has no stack to speak of)


def loop_class(cc, words):
    """The record loop a program takes, by the decoder's facts: the chain loop if rm_program_info calls the program without its
    tags a chain; the tree loop for any other untagged program of spheres and boxes under Union / Subtraction; the general
    loop for everything else (a Material tag is an extension node: a tagged program that is no chain takes the general loop)."""
    if renderer.program_info(cc, words)["is_chain"] == 1:
        return "chain"
    return "tree" if set(opcodes(cc, words)) <= set(CORE) else "general"


def _kinds(ud, limits, cc, words):
    py, px = np.meshgrid(np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    return set(int(k) for k in np.unique(gbuffer_ref.per_sample(px.ravel(), py.ravel(), 5, ud, limits, cc, words, W, H)["kind"]))


_cases = {}


def case(oracle, cls, seed):
    """The case (class, seed) names: namespace of cls, seed, cc, words, info, limits, table (8 x 3), events, u (the oracle's
    Uniforms), ud (the same as the dict the numpy references take) and redraws (how many programs were turned down)."""
    if (cls, seed) in _cases:
        return _cases[cls, seed]
    rng = np.random.default_rng([_SALT[cls], seed])
    limits = (float(rng.choice([0.01, 0.2])), float(rng.choice([100.0, 6.0])), int(rng.choice([24, 64])))
    table = rng.uniform(0.0, 1.0, (8, 3)).astype(F)
    for redraws in range(1000):
        t = scenes._Tab()
        root = _BUILD[cls](rng, t)
        cc, words = oracle.serialize(t.nodes, root)
        words = np.asarray(words, dtype=np.uint32)
        if oracle.validate(cc, words)[0] != 0 or renderer.validate_program(cc, words)[0] != 0 or not has_class(cls, cc, words, seed):
            continue
        for _ in range(8):
            events = [(1, float(rng.uniform(-300, 300)), float(rng.uniform(-140, 140))), (2, float(rng.uniform(-60, 150)), 0.0)]
            u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=events)
            ud = uniforms_dict(u)
            if _kinds(ud, limits, cc, words) == {0, 1, 2}:
                c = types.SimpleNamespace(cls=cls, seed=seed, cc=cc, words=words, info=renderer.program_info(cc, words),
                                          limits=limits, table=table, events=events, u=u, ud=ud, redraws=redraws)
                _cases[cls, seed] = c
                return c
    raise AssertionError("%s seed %d: no program in 1000 draws" % (cls, seed))


def describe(c):
    """What a failure message carries: enough to rebuild the case without the generator."""
    return "%sclass %s seed %d limits %s events %s info %s cmd_count %d words %s" % (
        getattr(c, "name", "") and c.name + ": ", c.cls, c.seed, c.limits, c.events, c.info, c.cc, [int(x) for x in c.words])


def points_of(c, n=18000):
    """About 20 000 points in sample_points' mix; never a multiple of 64 (a partial last wave)."""
    p = sample_points(c.cc, c.words, n, seed=c.seed + 1)
    return p if len(p) % 64 else np.ascontiguousarray(p[:-1])


def rays_of(c, n=2000):
    r = sample_rays(c.cc, c.words, n + (1 if n % 64 == 0 else 0), seed=c.seed + 2)
    assert len(r) % 64
    return r


# ---- constructed ties and NaN operands --------------------------------------------------------------------------------------------
# Every primitive parameter and every tie point below is exactly representable, and every transform keeps the tie locus exact:
# the translation moves x = 0.5 onto x = 0, the rotation is about the x axis (the formula leaves x untouched: its cross products
# with (ax, 0, 0) have no x component), the scale divides 0 by 2.
_SPH = ((0.25, -0.5, 0.125), 0.75)
_SPH_X = ((0.25, 0.0, 0.0), 0.75)                # centred on the x axis: its axis points stay exact under the rotation
_BOX = ((0.25, -0.5, 0.125), (0.5, 0.25, 0.75))
_PAIRS = {
    "union of duplicates": (scenes.UNION, None, "dup sphere"),
    "subtraction of duplicates": (scenes.SUBTRACTION, None, "dup sphere x"),
    "intersection of duplicates": (scenes.INTERSECTION, None, "dup sphere"),
    "smooth union of duplicates": (scenes.SMOOTH_UNION, 0.3, "dup sphere"),
    "union of mirror spheres": (scenes.UNION, None, "mirror"),
    "smooth union k=0 of mirror spheres": (scenes.SMOOTH_UNION, 0.0, "mirror"),
    "smooth union k<0 of mirror spheres": (scenes.SMOOTH_UNION, -0.25, "mirror"),
}
_PLACES = ("plain", "chain", "translation", "rotation", "scale")
_HALF = math.sqrt(0.5)


def _operand(t, shape, which):
    if shape == "dup sphere":
        return t.sphere(*_SPH)
    if shape == "dup sphere x":
        return t.sphere(*_SPH_X)
    return t.sphere((0.5 if which == "a" else -0.5, 0.0, 0.0), 0.75)


def _wrap(t, node, place):
    if place == "translation":
        return t.translation(node, (0.5, 0.25, -0.125))
    if place == "rotation":
        return t.rotation(node, (_HALF, _HALF, 0.0, 0.0))
    if place == "scale":
        return t.scale(node, 2.0)
    return node


def _tie_nodes(pair, place, part):
    """(nodes, root) of the program (part "pair") or of one operand in the pair's place (part "a" / "b")."""
    op, k, shape = _PAIRS[pair]
    t = scenes._Tab()
    if part == "pair":
        a = t.material(_operand(t, shape, "a"), 1)
        b = t.material(_operand(t, shape, "b"), 2)
        node = t.smooth_union(a, b, k) if op == scenes.SMOOTH_UNION else t.op(op, a, b)
    else:
        node = t.material(_operand(t, shape, part), 1 if part == "a" else 2)
    node = _wrap(t, node, place)
    if place == "chain" and part == "pair":      # the pair as the right operand of a left-deep chain of tagged leaves
        left = t.op(scenes.UNION, t.material(t.box((3.0, 0.0, 0.0), (0.25, 0.25, 0.25)), 3), t.material(t.sphere((0.0, 3.0, 0.0), 0.5), 4))
        node = t.op(scenes.UNION, left, node)
    if place == "scale" and part == "pair":      # a neighbour outside the scope: the factor of the Scale's pop decides who wins
        node = t.op(scenes.UNION, node, t.material(t.sphere((1.5, 0.5, 0.0), 1.0), 5))
    return t.nodes, node


def _grid(xs, ys, zs):
    return np.array([[x, y, z] for x in xs for y in ys for z in zs], dtype=F)


def _tie_points(pair, place):
    """(exact points on the tie locus, exact points off it), world coordinates."""
    op, k, shape = _PAIRS[pair]
    c = np.array(_SPH_X[0], dtype=F)
    s = F(2.0) if place == "scale" else F(1.0)
    shift = np.array((0.5, 0.25, -0.125) if place == "translation" else (0, 0, 0), dtype=F)
    lattice = _grid((-1.5, -0.25, 0.0, 0.5, 2.0), (-1.0, 0.0, 0.75), (-0.5, 0.0, 1.25))
    if shape == "mirror":                        # equal distances on the plane between the centres only
        on = _grid((0.0,), (-1.0, -0.5, 0.0, 0.25, 0.75, 2.0), (-1.5, -0.25, 0.0, 0.5, 1.0)) * s + shift
        off = lattice[lattice[:, 0] != 0] * s + shift
        return on.astype(F), off.astype(F)
    if op == scenes.SUBTRACTION:                 # a ties with -b where the common distance is 0: on the sphere, along the axes
        axes = (0,) if place == "rotation" else (0, 1, 2)      # (a rotated point is exact on the x axis only)
        on = np.array([c + F(0.75) * np.eye(3, dtype=F)[ax] * F(sg) for ax in axes for sg in (1, -1)], dtype=F) * s + shift
        return on.astype(F), (lattice * s + shift).astype(F)
    # duplicates under Union / Intersection / SmoothUnion tie everywhere but at a NaN coordinate (spheres: a box's distance
    # drops the NaN and would tie even there)
    return (lattice * s + shift).astype(F), np.zeros((0, 3), dtype=F)


def _tagged(cc, words, tag):
    """The command range (first, count) of the operand whose value Material(tag) tags."""
    idx = [i for i, op, p in commands(words, cc) if op == 300 and int(p.view(np.uint32)[0]) == tag]
    assert len(idx) == 1
    first, count = renderer.program_subtree(cc, words, idx[0])
    return first, count


def tie_cases(oracle):
    """The constructed programs: namespaces of name, cc, words, operand programs a and b ((cc, words) each), ties / others (exact
    points on and off the tie locus), first / second (the command ranges of the two tied operands), limits, table, u, ud and
    loop (loop_class: two tagged leaves under Union / Subtraction are a chain, every other one takes the general loop)."""
    table = np.random.default_rng(44000).uniform(0.0, 1.0, (8, 3)).astype(F)
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=STILL)
    out = []
    for pair in _PAIRS:
        for place in _PLACES:
            cc, words = oracle.serialize(*_tie_nodes(pair, place, "pair"))
            words = np.asarray(words, dtype=np.uint32)
            ties, others = _tie_points(pair, place)
            out.append(types.SimpleNamespace(
                name="%s, %s" % (pair, place), cc=cc, words=words, a=oracle.serialize(*_tie_nodes(pair, place, "a")),
                b=oracle.serialize(*_tie_nodes(pair, place, "b")), ties=ties, others=others, first=_tagged(cc, words, 1),
                second=_tagged(cc, words, 2), limits=(0.01, 100.0, 64), table=table, u=u, ud=uniforms_dict(u), cls="tie", seed=0,
                events=STILL, info=renderer.program_info(cc, words), mirror=_PAIRS[pair][2] == "mirror", loop=loop_class(cc, words)))
    return out


def nan_case(oracle):
    """A Scale by 0 next to healthy operands: inside the scope both operands are +inf (a tie) or NaN, what leaves it is NaN."""
    t = scenes._Tab()
    inner = t.scale(t.op(scenes.UNION, t.material(t.sphere(*_SPH), 1), t.material(t.box(*_BOX), 2)), 0.0)
    healthy = t.material(t.box((-0.5, 0.25, 0.0), (0.5, 0.75, 0.5)), 3)
    root = t.op(scenes.SUBTRACTION, t.op(scenes.UNION, t.op(scenes.UNION, t.material(inner, 4), healthy),
                                         t.material(t.scale(t.sphere((1.0, 0.0, 0.0), 0.5), 0.0), 5)),
                t.material(t.sphere((-0.5, 1.0, 0.0), 0.5), 6))
    cc, words = oracle.serialize(t.nodes, root)
    words = np.asarray(words, dtype=np.uint32)
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=STILL)
    return types.SimpleNamespace(name="scale by 0", cc=cc, words=words, limits=(0.01, 100.0, 64), cls="nan", seed=0, events=STILL,
                                 table=np.random.default_rng(44001).uniform(0.0, 1.0, (8, 3)).astype(F), u=u, ud=uniforms_dict(u),
                                 info=renderer.program_info(cc, words), first=_tagged(cc, words, 4), second=_tagged(cc, words, 3),
                                 loop=loop_class(cc, words))


def tie_point_set(c):
    """The points a constructed program is queried at: its exact tie points and the others, and sample_points' mix (near-surface
    points, centres, 1e-20 offsets, 1e4, inf / NaN / signed zeros)."""
    parts = [sample_points(c.cc, c.words, 1500, seed=5)]
    if hasattr(c, "ties"):
        parts = [c.ties, c.others] + parts
    p = np.ascontiguousarray(np.concatenate(parts).astype(F))
    return p if len(p) % 64 else np.ascontiguousarray(p[:-1])


def tie_rays(c):
    """Rays that start on the tie locus and stay on it: for the mirror pairs origins with x = 0 (0.5 under the translation)
    and directions with dx = 0, so every march position has that x exactly; for the others rays towards the tie points."""
    rng = np.random.default_rng(9)
    ties = c.ties if hasattr(c, "ties") else sample_points(c.cc, c.words, 40, seed=6)[:40]
    n = 300
    if getattr(c, "mirror", False):
        x = ties[0, 0]
        o = np.stack([np.full(n, x, dtype=F), rng.uniform(-4, 4, n).astype(F), rng.uniform(-4, 4, n).astype(F)], axis=1)
        tgt = np.stack([np.full(n, x, dtype=F), rng.uniform(-0.5, 0.5, n).astype(F), rng.uniform(-0.5, 0.5, n).astype(F)], axis=1)
        d = tgt - o
        assert np.all(d[:, 0] == 0)
    else:
        o = rng.uniform(-4, 4, (n, 3)).astype(F)
        d = ties[rng.integers(0, len(ties), n)] - o
    with np.errstate(all="ignore"):
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    rays = np.ascontiguousarray(np.concatenate([o, d], axis=1).astype(F))
    return np.ascontiguousarray(np.concatenate([rays, sample_rays(c.cc, c.words, 101, seed=8)]))


def shadow_threshold_case(oracle):
    """A box under the floor whose top face is exactly min_dist = 0.25 below it, one march step (every primary ray runs out and
    falls to the floor or the sky) and no shadow bias: the first shadow step of a floor point above the box returns exactly
    min_dist, and the steps after it move away from the box.  `light` names the lighting parameters."""
    t = scenes._Tab()
    root = t.box((0.0, -3.0, 0.0), (2.0, 1.25, 2.0))
    cc, words = oracle.serialize(t.nodes, root)
    words = np.asarray(words, dtype=np.uint32)
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=STILL)
    return types.SimpleNamespace(name="box 0.25 under the floor", cc=cc, words=words, limits=(0.25, 100.0, 1), cls="chain", seed=0,
                                 events=STILL, table=np.full((1, 3), 0.5, dtype=F), u=u, ud=uniforms_dict(u),
                                 info=renderer.program_info(cc, words), light=dict(shadow=1.0, ao=0.0, bias=0.0))
