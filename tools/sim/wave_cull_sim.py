#!/usr/bin/env python3
"""CPU simulation (numpy, binary64, statistics only): how many leaves does a wave of 64 rays marching in step have to evaluate per
iteration under different far tests?  A wave = one BATCH of the march kernel's ray pool: the sixteen AA samples of a 2x2 block of
pixels (lane: sample lane >> 2, pixel lane & 3 of the block), all rays advanced together, rays that end leave their lane idle.
The first march step is shared (every ray evaluates the scene at the camera: the kernel takes it once per frame), so a batch
starts at dist = f0 with threshold 2 |f0| and that evaluation is not counted.  Thresholds are 2 |F| without float margins.
  exact      a leaf is evaluated iff v_leaf <= thr for ANY live lane (per-lane, per-leaf test; the ideal of the threshold rule)
  pairs      rounds 1 and 2: bounding sphere per pair of consecutive leaves, then a test per box
  rho + T    one test per leaf for the whole wave, two reductions: |p* - c| - R - rho > max thr, p* the first live lane's
             position, rho the wave's radius about it
  one reduction, |p* - c| - R > S = max over live lanes (|p_l - p*| + thr_l), with |.| the
    L2       Euclidean norm (shipped until round 14: three multiply-adds and a square root per lane)
    L1       sum of the magnitudes (shipped: two additions)
    Linf     sqrt(3) times the largest magnitude
With --anchor (lattice programs) three more tables follow, for the anchored first step (rm_kernel_v5.h "Pruning"):
  per step index   leaves evaluated per wave-iteration under the shipped L1 rule and under the ideal -- the exact rule with the
                   threshold |F| at the point itself --, by the index of the march step (2 = a batch's first own step)
  anchor policies  a wave marches four batches of a tile in turn (batches w, w + 4, w + 8, w + 12 of the tile's claim order, w random;
                   n_batches / 2 tiles); the anchor is the first live lane's position and value at the first evaluation of the wave's
                   previous batch, thr = min(2 |f0|, |F_a| + |q - p_a|_1) at the first own step: none (shipped), taken inside the tile
                   (the wave's first batch of each tile as shipped), and carried over from the previously drawn tile (a random one)
  units per step   under "carried over", which the device matches: how many units a wave-step needs (the share of steps with 1, 2, ...)
                   and how many groups of four units are not empty -- what the single-unit path of rm_jit.h is sized by
usage: wave_cull_sim.py [scene] [W H] [n_batches] [--anchor]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scenes  # noqa: E402
from oracle import cbind  # noqa: E402

ANCHOR = "--anchor" in sys.argv
sys.argv = [a for a in sys.argv if a != "--anchor"]
scene = sys.argv[1] if len(sys.argv) > 1 else "g32"
W, H = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (1920, 1080)
NT = int(sys.argv[4]) if len(sys.argv) > 4 else 300
MAX_ITER, MIN_D, MAX_D = 256, 0.01, 100.0
nodes, root = getattr(scenes, scene)()


def flatten(nodes, root):
    """left-deep chain -> [(kind, params, op)] in evaluation order (op of leaf 0 = None)"""
    out = []

    def walk(i):
        kind, p, l, r = nodes[i]
        if kind in (scenes.SPHERE, scenes.BOX):
            return [(kind, p, None)]
        left = walk(l)
        right = walk(r)
        assert len(right) == 1, "chains only"
        return left + [(right[0][0], right[0][1], kind if kind != scenes.SMOOTH_UNION else ("m", p[0]))]
    return walk(root)


chain = flatten(nodes, root)
N = len(chain)
C = np.array([c[1][:3] for c in chain])
IS_S = np.array([c[0] == scenes.SPHERE for c in chain])
R_s = np.array([c[1][3] if c[0] == scenes.SPHERE else 0.0 for c in chain])
Hb = np.array([c[1][3:6] if c[0] == scenes.BOX else [0, 0, 0] for c in chain])
RB = np.where(IS_S, R_s, np.linalg.norm(Hb, axis=1))       # bounding radius


def leaf_values(p):     # p: (n,3) -> (n,N)
    d = p[:, None, :] - C[None]
    vs = np.linalg.norm(d, axis=2) - R_s[None]
    q = np.abs(d) - Hb[None]
    vb = np.linalg.norm(np.maximum(q, 0), axis=2) + np.minimum(q.max(axis=2), 0)
    return np.where(IS_S[None], vs, vb)


def fold(v):
    acc = v[:, 0].copy()
    for i in range(1, N):
        op = chain[i][2]
        if op == scenes.UNION:
            acc = np.minimum(acc, v[:, i])
        elif op == scenes.SUBTRACTION:
            acc = np.maximum(acc, -v[:, i])
        else:
            k = op[1]
            h = np.maximum(k - np.abs(acc - v[:, i]), 0) / k
            acc = np.minimum(acc, v[:, i]) - h * h * k * 0.25
    return acc


u, pos, q, orb = cbind.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
inv_proj = np.array(list(u.inv_proj)).reshape(4, 4).T
inv_view = np.array(list(u.inv_view)).reshape(4, 4).T
ro = (inv_view @ np.array([0, 0, 0, 1.0]))[:3]


def rays(px, py, s):
    i, j = s // 4, s % 4
    ox = ((i + 0.5) / 4 - 0.5) / W * 2.0
    oy = ((j + 0.5) / 4 - 0.5) / H * 2.0
    x = (px + 0.5) / W * 2 - 1 + ox
    y = 1 - (py + 0.5) / H * 2 + oy
    ndc = np.stack([x, y, -np.ones_like(x), np.ones_like(x)], axis=1)
    wv = (inv_view @ (inv_proj @ ndc.T)).T
    d = wv - np.concatenate([ro, [1.0]])[None]
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return d[:, :3]


pairs = [(2 * g, 2 * g + 1) for g in range(N // 2)]
PC = np.array([(C[a] + C[b]) / 2 for a, b in pairs])
PR = np.array([max(np.linalg.norm(C[a] - PC[g]) + RB[a], np.linalg.norm(C[b] - PC[g]) + RB[b]) for g, (a, b) in enumerate(pairs)])

rng = np.random.default_rng(1)
tiles_x, tiles_y = W // 8, H // 8
RULES = ("exact", "pairs", "rho+T", "L2", "L1", "Linf")
stat = dict.fromkeys(("iters", "live", "lane") + RULES, 0)
F0 = float(fold(leaf_values(ro[None]))[0])                 # the shared first step
done_tiles = 0
attempts = 0
lane = np.arange(64)
while done_tiles < NT and attempts < 40 * NT and MIN_D <= F0 <= MAX_D:
    attempts += 1
    tx, ty, blk = int(rng.integers(tiles_x)), int(rng.integers(tiles_y)), int(rng.integers(16))
    px = (tx * 8 + 2 * (blk & 3) + (lane & 1)).astype(float)
    py = (ty * 8 + 2 * (blk >> 2) + ((lane >> 1) & 1)).astype(float)
    d = np.concatenate([rays(px[4 * s:4 * s + 4], py[4 * s:4 * s + 4], s) for s in range(16)])
    # keep batches that are marched at all (the marched population is ~92 % hits); march first to classify
    sc = np.full(64, F0)
    live = np.ones(64, bool)
    hit = np.zeros(64, bool)
    hist = []
    thr = np.full(64, 2 * abs(F0))
    for it in range(1, MAX_ITER):
        if not live.any():
            break
        p = ro[None] + d * sc[:, None]
        v = leaf_values(p)
        F = fold(v)
        hist.append((live.copy(), p.copy(), v.copy(), thr.copy()))
        h = live & (F < MIN_D)
        hit |= h
        esc = live & ~h & (F > MAX_D)
        go = live & ~h & ~esc
        sc = np.where(go, sc + F, sc)
        thr = np.where(go, 2 * np.abs(F), thr)
        live = go
    if hit.sum() < 8:
        continue
    done_tiles += 1
    for live, p, v, thr in hist:
        l = live
        stat["iters"] += 1
        stat["live"] += l.sum()
        near = (v[l] <= thr[l][:, None])                 # (n_live, N)
        stat["lane"] += near.sum() / l.sum()
        stat["exact"] += near.any(axis=0).sum()
        # rounds 1 and 2: pair spheres, then boxes individually
        dp = np.linalg.norm(p[l][:, None, :] - PC[None], axis=2) - PR[None]
        pnear = (dp <= thr[l][:, None]).any(axis=0)
        cnt = 0
        for g, (a, b) in enumerate(pairs):
            if pnear[g]:
                for m in (a, b):
                    if IS_S[m]:
                        cnt += 1
                    else:
                        cnt += int(near[:, m].any())
        if N % 2:
            cnt += int(near[:, N - 1].any())
        stat["pairs"] += cnt
        # the wave rules: reference = first live lane
        pl, tl = p[l], thr[l]
        e = np.abs(pl - pl[0][None])
        gap = np.linalg.norm(C - pl[0][None], axis=1) - RB
        l2 = np.sqrt((e * e).sum(axis=1))
        stat["rho+T"] += (gap - l2.max() <= tl.max()).sum()
        stat["L2"] += (gap <= (l2 + tl).max()).sum()
        stat["L1"] += (gap <= (e.sum(axis=1) + tl).max()).sum()
        stat["Linf"] += (gap <= (np.sqrt(3.0) * e.max(axis=1) + tl).max()).sum()
it = max(stat["iters"], 1)
print("%s %dx%d: %d batches (2x2 pixels x 16 samples), %d wave-iterations after the shared first step (f0 = %.4f), lane occupancy %.2f" % (
    scene, W, H, done_tiles, stat["iters"], F0, stat["live"] / (64.0 * it)))
print("leaves of %d evaluated per wave-iteration: per-lane average %.2f" % (N, stat["lane"] / it))
for rule, label in (("exact", "exact per-lane union (ideal)"), ("pairs", "pair + box tests per lane (rounds 1, 2)"), ("rho+T", "rho + T, two reductions"),
                    ("L2", "L2 reach, one reduction"), ("L1", "L1 reach, one reduction (shipped)"), ("Linf", "sqrt(3) Linf reach, one reduction")):
    print("  %-42s %.2f" % (label, stat[rule] / it))

# ---- the anchored first step: leaves per step index, and what an anchor from the wave's previous batch saves ---------------
if ANCHOR and MIN_D <= F0 <= MAX_D and not any(isinstance(c[2], tuple) for c in chain):
    CLAIM = [(0xEDB87421A965FC30 >> (4 * k)) & 15 for k in range(16)]   # k-th batch of a tile's pool -> its 2x2 block (rm_kernel_v5.h)

    def march_batch(tx, ty, blk):
        """the own steps of one batch, [(live, p, v, F, thr)], or None when fewer than 8 of its rays hit (as above)"""
        px = (tx * 8 + 2 * (blk & 3) + (lane & 1)).astype(float)
        py = (ty * 8 + 2 * (blk >> 2) + ((lane >> 1) & 1)).astype(float)
        d = np.concatenate([rays(px[4 * s:4 * s + 4], py[4 * s:4 * s + 4], s) for s in range(16)])
        sc, live, hit, thr, steps = np.full(64, F0), np.ones(64, bool), np.zeros(64, bool), np.full(64, 2 * abs(F0)), []
        for it in range(1, MAX_ITER):
            if not live.any():
                break
            p = ro[None] + d * sc[:, None]
            v = leaf_values(p)
            F = fold(v)
            steps.append((live.copy(), p, v, F, thr.copy()))
            h = live & (F < MIN_D)
            hit |= h
            go = live & ~h & ~(F > MAX_D)
            sc = np.where(go, sc + F, sc)
            thr = np.where(go, 2 * np.abs(F), thr)
            live = go
        return steps if hit.sum() >= 8 else None

    def l1_mask(live, p, thr):
        pl, tl = p[live], thr[live]
        gap = np.linalg.norm(C - pl[0][None], axis=1) - RB
        return gap <= (np.abs(pl - pl[0][None]).sum(axis=1) + tl).max()

    def l1_count(live, p, thr):
        return int(l1_mask(live, p, thr).sum())

    def anchored(thr, p, anchor):
        return thr if anchor is None else np.minimum(thr, abs(anchor[1]) + np.abs(p - anchor[0][None]).sum(axis=1))

    rng = np.random.default_rng(2)
    by_step = {}                                     # step index -> [shipped L1, ideal, wave-iterations]
    POLICIES = ("shipped", "inside the tile", "carried over")
    first = dict.fromkeys(POLICIES, 0)
    total = dict.fromkeys(POLICIES, 0)
    n_first, tiles, attempts, carried = 0, 0, 0, None
    units_hist, groups_hist = {}, {}                 # "carried over" (the device's policy): units a wave-step needs, non-empty groups of four
    while tiles < max(NT // 2, 1) and attempts < 40 * NT:
        attempts += 1
        tx, ty, w0 = int(rng.integers(tiles_x)), int(rng.integers(tiles_y)), int(rng.integers(4))
        inside, marched = None, False
        for k in range(w0, 16, 4):
            steps = march_batch(tx, ty, CLAIM[k])
            if steps is None:
                continue
            marched = True
            for idx, (live, p, v, F, thr) in enumerate(steps):
                n = l1_count(live, p, thr)
                row = by_step.setdefault(idx + 2, [0, 0, 0])
                row[0] += n
                row[1] += int((v[live] <= np.abs(F[live])[:, None]).any(axis=0).sum())
                row[2] += 1
                for pol, anchor in zip(POLICIES, (None, inside, carried)):
                    m = n if idx > 0 or anchor is None else l1_count(live, p, anchored(thr, p, anchor))
                    total[pol] += m
                    if idx == 0:
                        first[pol] += m
                need = l1_mask(live, p, thr if idx > 0 or carried is None else anchored(thr, p, carried))
                units_hist[int(need.sum())] = units_hist.get(int(need.sum()), 0) + 1
                g = int(sum(need[k4:k4 + 4].any() for k4 in range(0, N, 4)))
                groups_hist[g] = groups_hist.get(g, 0) + 1
            n_first += 1
            live, p, v, F, thr = steps[0]
            k0 = int(np.argmax(live))
            inside = carried = (p[k0].copy(), float(F[k0]))
        tiles += int(marched)
    print("anchored first step: %d tiles, %d marched batches, one wave of four batches per tile" % (tiles, n_first))
    print("  step   wave-iterations   shipped L1   ideal (thr = |F| at the point)")
    for idx in sorted(by_step)[:14]:
        a, b, n = by_step[idx]
        print("  %4d   %15d   %10.2f   %5.2f" % (idx, n, a / n, b / n))
    n_all = sum(r[2] for r in by_step.values())
    print("   all   %15d   %10.2f   %5.2f" % (n_all, sum(r[0] for r in by_step.values()) / n_all, sum(r[1] for r in by_step.values()) / n_all))
    print("  share of the first own step in the shipped rule's leaf evaluations: %.1f %%" % (100.0 * first["shipped"] / total["shipped"]))
    print("  anchor policy      first own step, leaves of %d   all march-step leaf evaluations" % N)
    for pol in POLICIES:
        print("  %-16s   %28.2f   %8d (%+.1f %%)" % (pol, first[pol] / max(n_first, 1), total[pol], 100.0 * (total[pol] / total["shipped"] - 1.0)))
    # what a march step pays to find its units (rm_jit.h "Single-unit steps"): how many it needs, in how many groups of four
    n_steps = sum(units_hist.values())
    print("  units needed per wave-step (carried over), %d wave-steps:" % n_steps)
    print("    units   share of steps")
    for k in sorted(units_hist)[:8]:
        print("    %5d   %5.1f %%" % (k, 100.0 * units_hist[k] / n_steps))
    print("    non-empty groups of four:  " + "  ".join("%d: %.0f %%" % (k, 100.0 * groups_hist[k] / n_steps) for k in sorted(groups_hist)))

# ---- programs that blend: the local rule, per lane and through the wave's ball -----------------------------------------
if any(isinstance(c[2], tuple) for c in chain):
    RIN = np.where(IS_S, R_s, Hb.min(axis=1))
    KS = np.array([c[2][1] if isinstance(c[2], tuple) else 0.0 for c in chain])
    KMAX = KS.max()
    ISSUB = np.array([c[2] == scenes.SUBTRACTION for c in chain])
    st2 = {"iters": 0, "lane_local": 0, "union_local": 0, "ball_seq": 0, "ball_par": 0, "lane_restart": 0, "union_restart": 0}
    rng = np.random.default_rng(1)
    done = 0
    while done < NT:
        tx, ty = int(rng.integers(tiles_x)), int(rng.integers(tiles_y))
        s = int(rng.integers(16))
        px = (tx * 8 + np.arange(64) % 8).astype(float)
        py = (ty * 8 + np.arange(64) // 8).astype(float)
        d = rays(px, py, s)
        sc = np.zeros(64); live = np.ones(64, bool); hit = np.zeros(64, bool); hist = []
        for it in range(MAX_ITER):
            if not live.any():
                break
            p = ro[None] + d * sc[:, None]
            v = leaf_values(p)
            # per-lane fold with per-unit accumulators
            accs = np.zeros((64, N)); acc = v[:, 0].copy(); accs[:, 0] = acc
            for i in range(1, N):
                accs[:, i] = acc            # accumulator the unit meets
                op = chain[i][2]
                if op == scenes.UNION: acc = np.minimum(acc, v[:, i])
                elif op == scenes.SUBTRACTION: acc = np.maximum(acc, -v[:, i])
                else:
                    k = op[1]; h = np.maximum(k - np.abs(acc - v[:, i]), 0) / k
                    acc = np.minimum(acc, v[:, i]) - h * h * k * 0.25
            F = acc
            hist.append((live.copy(), p.copy(), v.copy(), accs.copy()))
            h_ = live & (F < MIN_D); hit |= h_
            esc = live & ~h_ & (F > MAX_D); go = live & ~h_ & ~esc
            sc = np.where(go, sc + F, sc); live = go
        if hit.sum() < 8:
            continue
        done += 1
        for live, p, v, accs in hist:
            l = live & hit
            if not l.any():
                continue
            st2["iters"] += 1
            vl, al = v[l], accs[l]
            # local rule per lane: unit needed unless v >= acc + k (U/M) or v + acc >= 0 (SUB); unit 0 always
            need = np.ones_like(vl, bool)
            need[:, 1:] = np.where(ISSUB[None, 1:], vl[:, 1:] + al[:, 1:] < 0, vl[:, 1:] < al[:, 1:] + KS[None, 1:])
            st2["lane_local"] += need.sum() / l.sum()
            st2["union_local"] += need.any(axis=0).sum()
            # restart per lane: last U/M unit with v <= acc - k; units before it are dead
            rs = (~ISSUB[None, :]) & (vl <= al - KS[None, :]); rs[:, 0] = False
            jstar = np.where(rs.any(axis=1), N - 1 - np.argmax(rs[:, ::-1], axis=1), 0)
            need_r = need & (np.arange(N)[None, :] >= jstar[:, None])
            st2["lane_restart"] += need_r.sum() / l.sum()
            st2["union_restart"] += need_r.any(axis=0).sum()
            # the wave's ball
            pl = p[l]; pc = pl[0]
            rho = np.linalg.norm(pl - pc[None], axis=1).max()
            D = np.linalg.norm(C - pc[None], axis=1)
            L = D - RB - rho; Hh = D + rho - RIN
            # sequential bounds
            needs = [True]; alo, ahi = L[0], Hh[0]
            for uix in range(1, N):
                if ISSUB[uix]:
                    if L[uix] + alo >= 0: needs.append(False)
                    else:
                        needs.append(True); ahi = max(ahi, -L[uix]); alo = max(alo, -Hh[uix])
                else:
                    k = KS[uix]
                    if L[uix] >= ahi + k: needs.append(False)
                    elif Hh[uix] <= alo - k:
                        needs = [False] * len(needs) + [True]; alo, ahi = L[uix], Hh[uix]
                    else:
                        needs.append(True); ahi = min(ahi, Hh[uix]); alo = min(alo, L[uix]) - k / 4
            st2["ball_seq"] += sum(needs)
            # parallel: prefix minima, chain lemma for the lower bound, subtractions assumed skippable (checked)
            Hm = np.where(ISSUB, np.inf, Hh); Lm = np.where(ISSUB, np.inf, L)
            ahi_p = np.concatenate([[np.inf], np.minimum.accumulate(Hm)[:-1]])
            alo_p = np.concatenate([[np.inf], np.minimum.accumulate(Lm)[:-1]]) - KMAX
            skip = np.where(ISSUB, L + alo_p >= 0, L >= ahi_p + KS); skip[0] = False
            rst = (~ISSUB) & (Hh <= alo_p - KS); rst[0] = False
            r = (N - 1 - np.argmax(rst[::-1])) if rst.any() else 0
            needp = ~skip; needp[:r] = False
            bad_sub = np.where(ISSUB & ~skip & (np.arange(N) >= r))[0]
            if len(bad_sub):
                needp[bad_sub[0]:] = True
            st2["ball_par"] += needp.sum()
    it = st2["iters"]
    print("blend, units of %d needed per wave-iteration: local rule per lane %.2f, union over the wave %.2f | with restarts per lane %.2f, union %.2f | ball, sequential bounds %.2f | ball, parallel bounds %.2f"
          % (N, st2["lane_local"] / it, st2["union_local"] / it, st2["lane_restart"] / it, st2["union_restart"] / it, st2["ball_seq"] / it, st2["ball_par"] / it))
