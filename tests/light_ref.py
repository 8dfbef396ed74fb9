"""The lighting contract of DESIGN.md section 13 in numpy: what rm_draw_lit must write, to the last bit.

TEST INFRASTRUCTURE, written from the text of section 13 and not from the kernel.  It stands on the numpy oracle's map_scene,
fmin and fmax (oracle/rm_oracle_np.py) and restates everything else: rays, march, taps, shadow, occlusion, floor, resolve.
Every numpy ufunc on float32 arrays is one binary32 operation per element, sqrt and / are correctly rounded, nothing is fused.

render(...) returns (frame, evaluations); render_pixels(px, py, ...) the same for chosen pixels only.  `evaluations` counts the
map_scene evaluations of each pixel: march steps, the four taps, the material walk of a tagged program, shadow steps, AO taps
(render_pixels(..., detail=True) also returns them per sample ray and per kind: {kind: (n, 16) array}, kinds PHASES)."""
import numpy as np

from oracle import rm_oracle_np as onp

F = np.float32
NAMES = ("pos_x", "pos_y", "pos_z", "shadow", "shadow_softness", "bias", "shadow_max_t", "shadow_steps", "ao", "ao_step",
         "ao_falloff", "ao_scale", "ao_taps")          # enum rm_light, in order
DEFAULTS = (2.0, -5.0, 3.0, 1.0, 8.0, 0.02, 20.0, 64.0, 1.0, 0.1, 0.75, 1.5, 5.0)
IDENTITY = dict(shadow=0.0, ao=0.0)
PHASES = ("march", "taps", "walk", "shadow", "ao")


def params(**named):
    """The 13 parameters as float32: the defaults with the named ones replaced (pos=(x, y, z) names the first three)."""
    p = np.array(DEFAULTS, dtype=F)
    if "pos" in named:
        p[0:3] = named.pop("pos")
    for k, v in named.items():
        p[NAMES.index(k)] = v
    return p


def _normalize3(x, y, z):
    l = np.sqrt((x * x + y * y) + z * z)
    return x / l, y / l, z / l


def _matvec(m, x, y, z, w):
    return tuple(((m[0 + r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] * w for r in range(4))


def shadow(cc, words, limits, p, ox, oy, oz, lx, ly, lz):
    """shadow(o, l) for arrays of rays -> (sh, evaluations)."""
    min_dist, max_dist = F(limits[0]), F(limits[1])
    k, max_t, steps = p[4], p[6], int(p[7])
    n = ox.shape[0]
    res = np.ones(n, dtype=F)
    t = np.zeros(n, dtype=F)
    evals = np.zeros(n, dtype=np.int64)
    alive = np.arange(n)
    for _ in range(steps):
        if alive.size == 0:
            break
        ta = t[alive]
        h = onp.map_scene(cc, words, max_dist, ox[alive] + lx[alive] * ta, oy[alive] + ly[alive] * ta, oz[alive] + lz[alive] * ta)
        evals[alive] += 1
        hit = h < min_dist
        res[alive[hit]] = F(0)                      # res = 0; stop
        idx, hg, tg = alive[~hit], h[~hit], ta[~hit]
        res[idx] = onp.fmin(res[idx], (k * hg) / tg)
        tn = tg + hg
        t[idx] = tn
        alive = idx[~(tn > max_t)]                  # if t > SHADOW_MAX_T: stop
    return onp.fmax(res, F(0)), evals


def ao(cc, words, limits, p, x, y, z, nx, ny, nz):
    """ao(p, n) for arrays of points -> ao (every point takes AO_TAPS evaluations)."""
    max_dist = F(limits[1])
    step, falloff, scale, taps = p[9], p[10], p[11], int(p[12])
    occ = np.zeros(x.shape[0], dtype=F)
    w = F(1)
    for i in range(1, taps + 1):
        h = step * F(i)
        d = onp.map_scene(cc, words, max_dist, x + nx * h, y + ny * h, z + nz * h)
        occ = occ + (h - d) * w
        w = w * falloff
    return onp.fmin(onp.fmax(F(1) - scale * occ, F(0)), F(1))


def _shade_sample(cc, words, limits, p, materials, ro, dx, dy, dz):
    """One ray per entry: (3, n) linear colour and the evaluations per kind, {kind of PHASES: (n,)}."""
    min_dist, max_dist, max_iter = F(limits[0]), F(limits[1]), int(limits[2])
    S, b, A = p[3], p[5], p[8]
    n = dx.shape[0]
    col = np.zeros((3, n), dtype=F)                 # sky rays stay (0, 0, 0)
    evals = {k: np.zeros(n, dtype=np.int64) for k in PHASES}
    # ---- the march, exactly ray_march's loop
    dist = np.zeros(n, dtype=F)
    alive = np.arange(n)
    hit_i, hit_p = [], []
    for _ in range(max_iter):
        if alive.size == 0:
            break
        d = dist[alive]
        qx, qy, qz = ro[0] + dx[alive] * d, ro[1] + dy[alive] * d, ro[2] + dz[alive] * d
        s = onp.map_scene(cc, words, max_dist, qx, qy, qz)
        evals["march"][alive] += 1
        hit = s < min_dist
        esc = ~hit & (s > max_dist)
        hit_i.append(alive[hit])
        hit_p.append((qx[hit], qy[hit], qz[hit]))
        go = ~(hit | esc)
        dist[alive[go]] = d[go] + s[go]
        alive = alive[go]
    hi = np.concatenate(hit_i) if hit_i else np.zeros(0, dtype=np.int64)
    is_hit = np.zeros(n, dtype=bool)
    is_hit[hi] = True
    if hi.size:
        # ---- surface hit at pos: taps, n, l, ndl exactly as ray_march / shade_hit
        x, y, z = (np.concatenate([q[k] for q in hit_p]) for k in range(3))
        e = F(0.0001)
        f0 = onp.map_scene(cc, words, max_dist, x + e, y + -e, z + -e)
        f1 = onp.map_scene(cc, words, max_dist, x + -e, y + -e, z + e)
        f2 = onp.map_scene(cc, words, max_dist, x + -e, y + e, z + -e)
        f3 = onp.map_scene(cc, words, max_dist, x + e, y + e, z + e)
        evals["taps"][hi] += 4
        nx, ny, nz = _normalize3(((f0 + -f1) + -f2) + f3, ((-f0 + -f1) + f2) + f3, ((-f0 + f1) + -f2) + f3)
        lx, ly, lz = _normalize3(x - p[0], y - p[1], z - p[2])
        ndl = (nx * lx + ny * ly) + nz * lz
        lit = ndl
        if S > 0:
            sh = np.ones(hi.size, dtype=F)
            m = ndl > 0
            sh[m], ev = shadow(cc, words, limits, p, (x + nx * b)[m], (y + ny * b)[m], (z + nz * b)[m], lx[m], ly[m], lz[m])
            evals["shadow"][hi[m]] += ev
            lit = ndl * (F(1) - S * (F(1) - sh))
        kd = onp.fmax(F(0.02), lit)
        if A > 0:
            kd = kd * (F(1) - A * (F(1) - ao(cc, words, limits, p, x, y, z, nx, ny, nz)))
            evals["ao"][hi] += int(p[12])
        if materials is None:
            albedo = np.tile(np.array([0.4, 0.7, 0.1], dtype=F), (hi.size, 1))
        else:                                       # the material the walk finds
            _, mat = onp.map_scene(cc, words, max_dist, x, y, z, want_material=True)
            evals["walk"][hi] += 1
            albedo = np.asarray(materials, dtype=F).reshape(-1, 3)[mat]
        for ch in range(3):
            col[ch, hi] = albedo[:, ch] * kd
    miss = np.nonzero(~is_hit)[0]
    if miss.size:
        # ---- floor hit at pf = (fx, -1.5, fz) with the reference colour c
        t = (F(-1.5) - ro[1]) / dy[miss]
        fl = miss[t > 0]
        t = t[t > 0]
        fx, fz = ro[0] + dx[fl] * t, ro[2] + dz[fl] * t
        fy = np.full(fl.size, F(-1.5))
        c = ((onp.f2i(np.rint(fx + F(0.5))) ^ onp.f2i(np.rint(fz + F(0.5)))) & 1).astype(F)
        g = F(0.2) * c
        rgb = [F(0.1) + g, F(0.1) + g, F(0.2) + g]
        if S > 0 or A > 0:
            f = np.ones(fl.size, dtype=F)
            if S > 0:
                lx, ly, lz = _normalize3(fx - p[0], fy - p[1], fz - p[2])
                sh = np.ones(fl.size, dtype=F)
                m = ly > 0
                sh[m], ev = shadow(cc, words, limits, p, fx[m], (fy + b)[m], fz[m], lx[m], ly[m], lz[m])
                evals["shadow"][fl[m]] += ev
                f = F(1) - S * (F(1) - sh)
            if A > 0:
                zero, one = np.zeros(fl.size, dtype=F), np.ones(fl.size, dtype=F)
                f = f * (F(1) - A * (F(1) - ao(cc, words, limits, p, fx, fy, fz, zero, one, zero)))
                evals["ao"][fl] += int(p[12])
            rgb = [ch * f for ch in rgb]
        for ch in range(3):
            col[ch, fl] = rgb[ch]
    return col, evals


def render_pixels(px, py, uniforms, limits, cmd_count, words, W, H, materials=None, light=None, detail=False):
    """Pixels (px[i], py[i]) of the W x H frame -> ((n, 4) float32, (n,) evaluations).  uniforms: dict of viewport_extent,
    inv_proj, inv_view (as oracle.rm_oracle_np.render takes it); light: the 13 parameters (None: the defaults)."""
    p = params() if light is None else np.asarray(light, dtype=F)
    assert p.shape == (13,)
    words = np.asarray(words, dtype=np.uint32)
    px, py = np.asarray(px, dtype=np.uint32), np.asarray(py, dtype=np.uint32)
    ve = np.asarray(uniforms["viewport_extent"], dtype=F)
    inv_proj, inv_view = np.asarray(uniforms["inv_proj"], dtype=F), np.asarray(uniforms["inv_view"], dtype=F)
    n = px.shape[0]
    with np.errstate(all="ignore"):
        ro = _matvec(inv_view, F(0), F(0), F(0), F(1))
        sx = ((px.astype(F) + F(0.5)) / F(W)) * F(2) - F(1)
        sy = F(1) - ((py.astype(F) + F(0.5)) / F(H)) * F(2)
        total = np.zeros((3, n), dtype=F)
        parts = {k: np.zeros((n, 16), dtype=np.int64) for k in PHASES}
        for s in range(16):                         # the sum order is part of the contract
            i, j = s // 4, s % 4
            ox = ((F(i) + F(0.5)) / F(4) - F(0.5)) / ve[0] * F(2)
            oy = ((F(j) + F(0.5)) / F(4) - F(0.5)) / ve[1] * F(2)
            pv = _matvec(inv_proj, sx + ox, sy + oy, np.full(n, F(-1)), np.full(n, F(1)))
            pw = _matvec(inv_view, *pv)
            d = [pw[k] - ro[k] for k in range(4)]
            ln = np.sqrt(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3])
            col, ev = _shade_sample(cmd_count, words, limits, p, materials, ro, d[0] / ln, d[1] / ln, d[2] / ln)
            total = total + np.sqrt(col)
            for k in PHASES:
                parts[k][:, s] = ev[k]
        out = np.empty((n, 4), dtype=F)
        for ch in range(3):
            out[:, ch] = total[ch] / F(16)
        out[:, 3] = F(1)
    evals = sum(parts[k].sum(axis=1) for k in PHASES)
    return (out, evals, parts) if detail else (out, evals)


def render(uniforms, limits, cmd_count, words, W, H, row0=0, rows=None, materials=None, light=None):
    """Rows [row0, row0 + rows) of the lit frame -> ((rows, W, 4) float32, (rows, W) evaluations)."""
    rows = H - row0 if rows is None else rows
    py, px = np.meshgrid(np.arange(row0, row0 + rows, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    out, evals = render_pixels(px.ravel(), py.ravel(), uniforms, limits, cmd_count, words, W, H, materials, light)
    return out.reshape(rows, W, 4), evals.reshape(rows, W)
