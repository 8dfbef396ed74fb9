"""The pruning threshold of a march step with its position term bounded along the ray (rm_kernel_v5.h "Pruning", the position
term along a ray): a binary32 restatement of the four device functions, one binary32 operation per
operation of the kernel and every multiply-add a single rounding (wave_reach_model.fma32), beside the old expression they
replace (anchor_ref.step_threshold), and the rays tests/test_step_thr_cpu.py marches with them.

    c0       = kPruneAbsUp * (prune_scale + |ro|_1) + 1e-30                       step_thr_c0        once per wave
    thr_base = fma(|sd|, kStepReach, c0)                                          step_thr_base      every step
    thr_base = fma(min(|f0| * 2.00002f, the anchored bound), 1 + 2^-22, c0)       handout_thr_base   when a ray is handed out
    thr      = fma(|sc|, kPruneRay, thr_base)                                     step_thr           every step, at q = ro + d sc
    old      = T + 4e-6f * (prune_scale + |q|_1),  T = |sd| * 2.00002f or the hand-out's minimum"""
import numpy as np

import anchor_ref as A
import cull_ref as R
from wave_reach_model import fma32

F = np.float32
K_PRUNE_ABS_UP = F(4.0001e-6)
K_PRUNE_RAY = F(6.9285e-6)
K_STEP_REACH = F(2.0000205)
K_STEP_OLD = F(2.00002)
K_HANDOUT = F(1.00000024)
C0_FLOOR = F(1.0e-30)
# what the derivation beside the code asks of the constants, as binary32 numbers
assert float(K_PRUNE_ABS_UP) >= float(A.K_PRUNE_ABS) * (1.0 + 2.5e-5)
assert float(K_PRUNE_RAY) >= float(A.K_PRUNE_ABS) * np.sqrt(3.0) * (1.0 + 4.2e-5)
assert float(K_STEP_REACH) == float(K_STEP_OLD) + 2.0 ** -21 and float(K_HANDOUT) == 1.0 + 2.0 ** -22


def step_thr_c0(ps, ro):
    with np.errstate(all="ignore"):
        return F(K_PRUNE_ABS_UP * F(F(ps) + A.l1(ro)) + C0_FLOOR)


def step_thr_base(sd, c0):
    return fma32(np.abs(np.asarray(sd, dtype=F)), K_STEP_REACH, c0)


def handout_thr_base(thr_base, c0):
    return fma32(thr_base, K_HANDOUT, c0)


def step_thr(thr_base, sc):
    return fma32(np.abs(np.asarray(sc, dtype=F)), K_PRUNE_RAY, thr_base)


def old_thr_base(sd):
    with np.errstate(all="ignore"):
        return (np.abs(np.asarray(sd, dtype=F)) * K_STEP_OLD).astype(F)


def point(ro, d, sc):
    """the step's own expression for its point: ro + d * sc, a product and a sum per coordinate"""
    with np.errstate(all="ignore"):
        return (np.asarray(ro, dtype=F) + (np.asarray(d, dtype=F) * np.asarray(sc, dtype=F)[..., None]).astype(F)).astype(F)


def directions(ro, centre, rng, n):
    """normalised binary32 directions from ro: a cone about the scene's centre (three quarters) and anywhere (the rest)"""
    fwd = R.unit(np.asarray(centre, dtype=np.float64) - np.asarray(ro, dtype=np.float64))[0]
    k = (3 * n) // 4
    d = np.concatenate([R.unit(fwd[None] + rng.normal(size=(k, 3)) * 0.4), R.unit(rng.normal(size=(n - k, 3)))])
    return d.astype(F)
