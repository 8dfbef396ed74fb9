// rm_kernel_v5.h -- kernel v5 "streamed ray pool" (gfx950, wave64).  Device code only.
//
// One workgroup of WPT waves owns an 8x8-pixel tile and the pool of its 1024 rays: a lane marches ONE
// ray at a time; when its ray ends, the lane is refilled (ballot + prefix count) with the next ray, so
// every trip through map_scene runs with (nearly) all 64 lanes live whatever the per-ray step counts
// are.  WHERE the expensive, branchy per-ray work runs:
//
//   produce  Ray generation (2 mat-vec + vec4 normalize: wgsl:52-62) and the exact miss test run
//            for 64 consecutive rays of the pool at a time with ALL lanes active, using scratch
//            registers only (the marching state of the lanes is not touched).  Rays that provably
//            miss the scene are shaded on the spot (res[r] = floor code); survivors are compacted
//            with ballot + prefix count into a per-wave READY ring in LDS (ray id + direction).
//   consume  A lane whose ray ended pops the next ready ray: four LDS reads.
//   shade    A finished ray pushes its shading inputs (hit: normal sum + position, miss:
//            direction) into a per-wave SHADE ring; it is flushed (all waiting entries shaded at
//            once, 2 normalizes = 6 correctly rounded divides + 2 sqrt per hit) when the next push
//            would not fit.
//
// In the retired v2-v4 kernels (DESIGN.md 5 keeps their numbers) these pieces ran inside the march loop
// under a sparse exec mask (typically 8-14 of 64 lanes) and cost ~25 % of all vector instructions; here
// they run at (nearly) full occupancy and the march loop is: evaluation point, map_scene, ~20 VALU of
// state update, three ballots.
// Both rings are private to a wave (no barrier; LDS executes a wave's accesses in order), the
// pool cursor and the result array are shared by the tile's waves.
//
// Miss test: spheres get a cone test, boxes a ray/slab test against the box inflated by the margin
// (min_dist + 1e-4 of the local coordinate scale; float error of positions and SDF values is ~1e-6 of
// that scale).
#pragma once
#include "rm_interp.h"
#include "rm_lds_layout.h"

namespace rmk {

// Structure-specialised evaluation (rm_jit.h): when a program's command sequence has been compiled
// into straight-line code by hipRTC, the generated translation unit defines this function and
// instantiates the kernel body with SPEC = true; the library's own build only declares it.
//   lp: the decoded program in LDS (RmRecord[n], 8 dwords each: parameters are read at fixed offsets)
//   thr, live: far-primitive pruning, see below
// LdsF: an explicit LDS (address space 3) pointer.  The body hands map_scene_spec a base that went through a
// v_mov_b32 in inline asm, so the compiler sees ONE vector register plus compile-time offsets and folds those into
// the ds_read offset fields.  With a scalar base, ROCm 7.2's compiler materialised every record address in an SGPR
// of its own (40 live scalars, spilled and re-read with v_readlane inside the march loop: +33 % kernel time); ROCm
// 7.0's did not.  The laundering makes both produce the same loop.
typedef const __attribute__((address_space(3))) float* LdsF;
RM_DEV LdsF lds_vector_base(const void* generic_lds_ptr) {
    const uint32_t s = (uint32_t)(__SIZE_TYPE__)(const __attribute__((address_space(3))) void*)generic_lds_ptr;
    uint32_t v;
    asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(s));
    return (LdsF)(__SIZE_TYPE__)v;  // LDS pointers are 32 bits wide; the widening only silences the host pass
}
// `need`: the units of the program (rm_units.h) some live lane may depend on, one bit each, from wave_cull_* below (all ones
// when the kernel does not cull); `live`: wave mask of the lanes whose value will be used
template <bool FAST>
RM_DEV float map_scene_spec(LdsF lp, float qx, float qy, float qz, unsigned long long need, unsigned long long live, SqrtGuard& tiny, uint32_t& n_eval);
#ifdef RM_JIT_UNIT_WALK
// map_scene_spec behind the single-unit path (rm_jit.h "Single-unit steps"): a step whose mask holds one unit evaluates that leaf
// at an LDS address computed from the bit's position instead of walking the tests of the straight-line code; the same value, bit
// for bit.  The march steps call this one.
template <bool FAST>
RM_DEV float map_scene_walk(LdsF lp, float qx, float qy, float qz, unsigned long long need, unsigned long long live, SqrtGuard& tiny, uint32_t& n_eval);
#define RM_MAP_SCENE_STEP map_scene_walk
#else
#define RM_MAP_SCENE_STEP map_scene_spec
#endif
#ifdef RM_JIT_MATERIAL_WALK
// The material walk of a tagged program as straight-line code (rm_jit.h generate_material_walk): which material does the
// surface at (x, y, z) carry.  mp: the tagged records in device memory (uniform addresses: scalar loads).
template <bool FAST>
RM_DEV uint32_t map_scene_material_spec(const RmRecord* __restrict__ mp, float qx, float qy, float qz, SqrtGuard& tiny);
#endif
#ifdef RM_JIT_TAPS4
// The four normal taps of a hit at c in one pass (rm_jit.h generate_map_scene_taps): f[t] = map_scene(c + k_t eps).
template <bool FAST>
RM_DEV void map_scene_taps(LdsF lp, float cx, float cy, float cz, unsigned long long need, unsigned long long live, SqrtGuard& tiny, float (&f)[4]);
#endif

// ---- Pruning of far primitives (exact) ----------------------------------------------------------------
// A tree of min / max / negation over leaf values is monotone in every leaf: as a function of one
// leaf's signed value t (t = v for a leaf the tree value F grows with, t = -v below an odd number of
// subtraction right-hand sides) it is  F(t) = max(lo, min(hi, t))  for some lo <= hi, or constant.
// Hence, if F is known to lie in [-thr, thr] and a leaf has v > thr, then t > thr >= F(t) forces
// hi < t (resp. t < -thr <= F(t) forces lo > t): F does not depend on that leaf any more and is
// unchanged -- bit for bit, min and max only select -- if the leaf value is replaced by +inf.  The
// generated code then skips the leaf: "acc = min(acc, +inf)" and "acc = max(acc, -inf)"
// leave acc alone; a leaf that is pushed becomes the constant +inf.
//
// thr comes from the previous evaluation of the same ray.  Every node type admitted here (sphere,
// box, capped cylinder; union, subtraction, intersection) is 1-Lipschitz in real arithmetic, so the
// value F' at the next point q' satisfies |F' - F| <= |q' - q|; with the evaluation error E of the
// float computation on both sides,  |F'_computed| <= |F_computed| + |q' - q| + 2E.
//   march step (wgsl:114): |q' - q| <= |sd| (|rd| <= 1)      -> thr = 2 |sd| (1 + 1e-5) + m
//   normal taps (wgsl:138-141): |q' - q_hit| = eps sqrt(3)    -> thr = |sd_hit| (1 + 1e-5) + 1.75e-4 + m
//   first evaluation of a ray                                 -> thr = +inf (nothing is skipped)
// m = 4e-6 (scene_scale + |ro|_1 + |q'|_1) covers 3E (E <= 4e-7 of that scale: a handful of binary32
// roundings of quantities no larger than it) plus the rounding of q' itself, with 3x to spare.
// Programs with a Plane (|n| arbitrary) or a SmoothUnion (not a lattice operator) are not pruned this way; programs that
// blend have rules of their own (below).
constexpr float kPruneAbs = 4.0e-6f;
// Anchored first step.  The inequality above never asks that q and q' lie on one ray: ANY pair (p_a, F_a = the value this launch
// computed at p_a) bounds the value at q' by |F_a| + |q' - p_a| + 2E.  The first own step of a ray that took the frame's shared
// step is anchored at the camera (F(ro) = f0, |q' - ro| <= |f0|): thr = 2 |f0|, larger than the scene for a camera that stands
// back from it -- nothing is skipped there.  But the wave has just evaluated the scene a few pixels away on the same start
// sphere: it keeps one such pair (ax, ay, az, aT), wave-uniform, taken from its first live lane at the first evaluation after
// it handed out rays, and a ray that takes the shared step afterwards gets
//     aT       = |F_a| (1 + 1e-5) + 4e-6 (scene_scale + |ro|_1 + |p_a|_1)                      (anchor_reach)
//     thr_base = min(2 |f0| (1 + 1e-5), fl(fl(l1) (1 + 1e-5) + aT)),   l1 = |q' - p_a|_1      (anchor_thr_base)
// to which the step adds its own position term m(q') -- or a bound of it, below -- as for every threshold.  Why that bounds |F'_computed|:
//   - p_a and q' are the binary32 points the evaluations ran AT (q' by the step's own expression, which with contraction off
//     gives the same bits here; were it an ulp off, m(q') covers the rounding of q' as it always did), so the real distance
//     between them is what counts, and |q' - p_a|_2 <= |q' - p_a|_1: the triangle inequality holds a fortiori with the L1 norm
//     (the choice of wave_cull_lattice: no square root);
//   - fl(l1): each of the three differences, and each of the two sums, is one rounding -- relative error 2^-24, none where it
//     underflows (sums and differences of binary32 numbers are exact there) --, so fl(l1) >= l1 (1 - 2^-24)^3 > l1 (1 - 1.8e-7);
//     the multiply-add rounds once more, fl(t) >= t (1 - 2^-24).  The factor 1.00001f (>= 1 + 9.9e-6 as a binary32 number) on
//     both l1 and |F_a| leaves 9.6e-6 (l1 + |F_a|) after these losses; the term aT adds beyond |F_a| loses 6e-8 of itself to
//     the last rounding, which its threefold reserve (next line) does not notice;
//   - the evaluation error at BOTH points: E(p_a) <= 4e-7 (scene_scale + |ro|_1 + |p_a|_1) sits in aT with its factor 4e-6,
//     E(q') in m(q') -- each term has one E to cover where the march step's single m covers three;
//   - non-finite inputs: a NaN F_a or a non-finite p_a makes aT NaN or +inf; a non-finite q' or an overflow makes l1, and so
//     t, +inf or NaN (inf - inf); `t < thr_base` is false for all of them and the camera's threshold stays.  A NaN thr_base
//     (f0 NaN) stays NaN.  No anchor yet: aT = +inf.
// The anchor is never reset between tiles (a far anchor loses the min: it can only fail to help) and lives in four scalar
// registers.  tools/sim/wave_cull_sim.py --anchor: leaves evaluated at the first own step of a batch 16.0 -> 2.7 of 16.
RM_DEV float anchor_reach(float px, float py, float pz, float sd, float prune_scale) {
    return __builtin_fabsf(sd) * 1.00001f + kPruneAbs * (prune_scale + ((__builtin_fabsf(px) + __builtin_fabsf(py)) + __builtin_fabsf(pz)));
}
RM_DEV float anchor_thr_base(float thr_base, float qx, float qy, float qz, float ax, float ay, float az, float aT) {
    const float l1 = (__builtin_fabsf(qx - ax) + __builtin_fabsf(qy - ay)) + __builtin_fabsf(qz - az);
    const float t = __builtin_fmaf(l1, 1.00001f, aT);
    return t < thr_base ? t : thr_base;  // NaN t: the old value stays
}
// The position term along a ray.  m(q') = 4e-6 (prune_scale + |q'|_1), prune_scale = scene_scale + |ro|_1, is there to cover
// evaluation error "with 3x to spare": any upper bound of it serves, and a march step has a cheap one.  Its point is
// q' = ro + d sc with |d|_2 <= 1 + 1e-5 (a normalised ray; the "|rd| <= 1" of the rule above), so
//     |q'|_1 <= |ro|_1 + |d|_1 |sc| <= |ro|_1 + sqrt(3) (1 + 1e-5) |sc|
// and the step's threshold is ONE multiply-add, thr = fma(|sc|, kPruneRay, thr_base), where it was five instructions (two sums
// of magnitudes, + prune_scale, * 4e-6, + thr_base), with the wave-uniform rest c0 >= 4e-6 (prune_scale + |ro|_1) carried
// inside thr_base: added where the bookkeeping forms it (a multiply-add in place of the multiply), and where a ray is handed out.
//     c0       = fl(fl(kPruneAbsUp * fl(prune_scale + fl(|ro|_1))) + 1e-30)                    (step_thr_c0, once per wave)
//                (a product and a sum, two roundings: both builds compile with -ffp-contract=off, build.py HIP_FLAGS and rm_jit.h
//                compile_options, and tests/step_thr_ref.py restates it so; contracted to one multiply-add it would lose one rounding
//                less, and every bound below holds for that form too)
//     thr_base = fma(|sd|, kStepReach, c0)                                                      (step_thr_base, every step)
//     thr_base = fma(min(2 |f0| (1 + 1e-5), the anchored bound), 1 + 2^-22, c0)                 (handout_thr_base, per ray)
//     thr      = fma(|sc|, kPruneRay, thr_base)                                                 (step_thr, every step)
// new >= old for every finite input, old = fl(T + M) with T = fl(|sd| 2.00002f) (or the hand-out's minimum, the same number on
// both sides) and M = fl(4e-6f fl(prune_scale + fl(|q'|_1))).  With u = 2^-24, every rounding to nearest and monotone, and an
// absolute error of at most 2^-150 where a PRODUCT lands among the denormals (sums are exact there):
//   - M: each coordinate fl(ro + fl(d sc)) is at most (|ro| + |d| |sc| (1 + u)) (1 + u), the two sums of |q'|_1, the sum with
//     prune_scale and the product add (1 + u) each: M <= 4e-6f (prune_scale + |ro|_1 + |d|_1 |sc|) (1 + u)^6 + 2^-150, and
//     (1 + u)^6 < 1 + 3.6e-7;
//   - c0: the two sums of |ro|_1, the sum with prune_scale and the product lose (1 - u) each, the last sum is monotone:
//     c0 >= kPruneAbsUp (prune_scale + |ro|_1) (1 - 2.4e-7) - 2^-150 and c0 >= 1e-30 (1 - u).  kPruneAbsUp >= 4e-6f (1 + 2.5e-5) as
//     binary32 numbers: a hundred times what the two lines lose together;
//   - kPruneRay = 6.9285e-6f >= 4e-6f sqrt(3) (1 + 4.2e-5): |d|_1 <= sqrt(3) |d|_2, the 1e-5 of |d|_2, the 3.6e-7 of M, 3e-5 left over;
//   - thr_base, step: fma(|sd|, kStepReach, c0) >= (|sd| kStepReach + c0) (1 - u) - 2^-150 with kStepReach = 2.0000205f =
//     2.00002f (1 + 4 u): (1 + 4 u) (1 - u) > 1 + u, so it is at least |sd| 2.00002f (1 + u) + c0 (1 - u) - 2^-150
//     >= T + c0 (1 - u) - 2^-149.  (Two units in the last place on the factor: 2.4e-7 of the threshold.  Without them the
//     rounding of the LARGE term could eat the small one: u T against c0.)  Hand-out: the same with the factor 1 + 2^-22
//     = 1 + 4 u on the minimum, T itself: >= T + c0 (1 - u) - 2^-150; +inf stays +inf;
//   - together, in real numbers, |sc| kPruneRay + thr_base >= T + M: the reserves above against the losses, the 1e-30 in c0
//     against the 2^-150s; the last multiply-add and the old last sum each round once, monotonically: thr >= old.
// Hence every bound proven for the old threshold holds for this one, the anchored form included (its minimum is taken first,
// on the same numbers as before: anchor_reach and anchor_thr_base are untouched and c0 is added to the result).  It is larger
// by at most 4e-6 (|ro|_1 + |d|_1 |sc| - |q'|_1) + 3e-5 m + 2.4e-7 T: 1e-5 .. 1e-4 for the metric camera against thresholds
// of 1e-2 .. 1 -- the leaves evaluated do not move (profiles/r25_step_front_end_ab.txt).
// Non-finite inputs: a non-finite sc makes |sc| kPruneRay +inf or NaN, and thr with it (thr_base is never -inf).  A non-finite
// d with a finite sc leaves thr finite where the old form, which read q', did not -- but thr is only ever read by the
// wave-level masks, at the same q': a non-finite coordinate of a live lane gives sl = +inf or NaN there (wave_cull_lattice,
// "Slack") and no comparison holds.  A NaN sd, or a NaN or infinite f0, goes through both multiply-adds as NaN or +inf; a
// ray that does not take the shared step starts from +inf.
// The taps keep the old term: their point is not on a ray, and they run once per hit.  So does the general interpreter loop,
// which reads the threshold without keeping an anchor: the form above is compiled in where ANCHOR is (rm_render_v5_body).
// tests/step_thr_ref.py restates the four functions in binary32; tests/test_step_thr_cpu.py holds new >= old, the bound on the
// value and the non-finite cases.
constexpr float kPruneAbsUp = 4.0001e-6f;
constexpr float kPruneRay = 6.9285e-6f;
constexpr float kStepReach = 2.0000205f;
RM_DEV float step_thr_c0(float prune_scale, float rox, float roy, float roz) {
    return kPruneAbsUp * (prune_scale + ((__builtin_fabsf(rox) + __builtin_fabsf(roy)) + __builtin_fabsf(roz))) + 1.0e-30f;
}
RM_DEV float step_thr_base(float sd, float c0) { return __builtin_fmaf(__builtin_fabsf(sd), kStepReach, c0); }
RM_DEV float handout_thr_base(float thr_base, float c0) { return __builtin_fmaf(thr_base, 1.00000024f, c0); }
RM_DEV float step_thr(float thr_base, float sc) { return __builtin_fmaf(__builtin_fabsf(sc), kPruneRay, thr_base); }
// The thresholds are kept (a register per ray, |sd| of a hit in its hit-buffer entry) by the generated kernels compiled
// with pruning and by the library's interpreter kernels
#if defined(RM_JIT_PRUNE_ON) || !defined(RM_JIT_TU)
#define RM_PRUNE_PLUMBING 1
#endif

// ---- Wave-level culling: WHICH units does this wave have to evaluate ----------------------------------------------------
// Rounds 1 and 2 tested every pair of leaves (and every box) against every lane's own threshold, 64 lanes wide, at every
// evaluation: ~120 of the ~330 vector instructions of a march step of the metric scene.  But the 64 rays of a wave come
// from one 8x8-pixel tile and march in step: their positions lie in a small ball.  So the test is TRANSPOSED -- lane u
// looks at unit u (rm_units.h; its bounded stand-in sits in LDS behind the program, RmDecoded::units) and decides for the
// whole wave:
//   p*   the position of the first live lane,  rho >= max over live lanes |p_l - p*|   (one wave reduction)
//   unit u with centre c, outer radius R, inner radius r_in:  for every live lane
//        L_u = |p* - c| - R - rho  <=  value_u(p_l)  <=  |p* - c| + rho - r_in = H_u      (triangle inequality)
// LATTICE programs (threshold rule above): unit u is far for lane l when |p* - c| - R - |p_l - p*| > thr_l; for the whole wave
//   when |p* - c| - R > S = max over live lanes (|p_l - p*| + thr_l) -- one reduction (the first form took rho and T = max thr_l
//   separately: L_u > T), with |p_l - p*| in the L1 norm (wave_cull_lattice below).  A CPU simulation of the metric frame
//   (tools/sim/wave_cull_sim.py; batches of 2x2 pixels x 16 samples) has the rho + T form evaluate 3.62 of 16 leaves per step, S with the
//   L2 norm 3.60, with the L1 norm 3.63, where the per-lane pair tests evaluate 4.54 and a per-lane, per-leaf test 3.09.
// Programs that BLEND, top-level chain (rm_units.h).  With a_hi(u) = min over the Union / SmoothUnion units j < u of H_j
//   (the accumulator a unit meets is at most the smallest leaf blended in so far) and a_lo(u) = min_j L_j - kmax (a chain
//   of blends never falls more than the largest k below its smallest leaf: rm_decode.h [*]; Subtraction and Intersection
//   only raise it) -- two prefix minima over the lanes --:
//        Union / SmoothUnion(k)   L_u >= a_hi + k + m   -> the operator returns the accumulator (h = 0): skipped
//                                 H_u <= a_lo - k - m   -> it returns the leaf: RESTART, every unit in front of u is dead
//        Subtraction              L_u + a_lo >= m       -> max(acc, -v) = acc: skipped
//        Intersection             H_u <= a_lo - m       -> max(acc, v) = acc: skipped
//   a_hi is only an upper bound while no Subtraction / Intersection has raised the accumulator: the first one that is not
//   skipped (and any opaque unit, behind which nothing is known) POISONS the rules -- every unit behind it is evaluated.
//   Same simulation, config 3: 4.4 of 16 units per step against 7.2 for the per-lane rule of the first half of this round.
// All comparisons fail on a NaN (the unit is evaluated); m is the margin of the threshold rule at p*, with rho added.
// Cost: ~30 vector instructions per evaluation for a lattice program, ~100 for a blending one, whatever the number of units.
#define RM_DPP(old, src, ctrl) ((uint32_t)__builtin_amdgcn_update_dpp((int)(old), (int)(src), (ctrl), 0xF, 0xF, false))
// largest value over the wave, wave-uniform (all 64 lanes must be active; lanes without a value pass 0).  Four DPP steps
// leave every row of 16 lanes with its maximum (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror), two
// row broadcasts carry it on to lane 63 (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3; a lane without a source
// gets 0), one v_readlane fetches it.  (The first form read the four rows' maxima with four v_readlane and combined them with
// three s_max_u32: instructions of the 4.3-cycle kind -- a CU has ONE scalar unit for its four SIMDs,
// profiles/r03_ubench_scalar_issue_cycles.txt -- where a DPP step is an ordinary vector instruction.)
RM_DEV uint32_t wave_max_u32(uint32_t v) {
    uint32_t t;
    t = RM_DPP(0u, v, 0xB1); v = t > v ? t : v;
    t = RM_DPP(0u, v, 0x4E); v = t > v ? t : v;
    t = RM_DPP(0u, v, 0x141); v = t > v ? t : v;
    t = RM_DPP(0u, v, 0x140); v = t > v ? t : v;
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false); v = t > v ? t : v;
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false); v = t > v ? t : v;
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// minimum over the lanes BELOW this one (+inf for lane 0); all 64 lanes active.  row_shr:1,2,3, row_shr:4, row_shr:8 scan a row
// of 16, row_bcast:15 and row_bcast:31 carry the rows' totals on (a lane without a source keeps its value; min is idempotent, so
// it does not matter that a total may be counted twice); then one shift by a lane across the whole wave (wave_shr:1).
// Written as v_min_f32_dpp: through __builtin_fminf and update_dpp every step was four instructions (the identity moved in, the
// DPP move, a canonicalising v_max, the v_min) and the last shift a ds_bpermute -- 65 vector instructions for the two scans of
// a blending chain's mask where 16 do.  (v_min_f32 drops a NaN operand like fminf does; s_nop 1: a DPP source written by the
// previous vector instruction needs two wait states, and the compiler does not look inside an asm.)
RM_DEV float wave_exclusive_min(float x) {
    float s = x;
    asm volatile("s_nop 1\n\tv_min_f32_dpp %0, %1, %0 row_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(s) : "v"(x));
    asm volatile("v_min_f32_dpp %0, %1, %0 row_shr:2 row_mask:0xf bank_mask:0xf" : "+v"(s) : "v"(x));
    asm volatile("v_min_f32_dpp %0, %1, %0 row_shr:3 row_mask:0xf bank_mask:0xf" : "+v"(s) : "v"(x));
    asm volatile("s_nop 1\n\tv_min_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf" : "+v"(s));
    asm volatile("s_nop 1\n\tv_min_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf" : "+v"(s));
    asm volatile("s_nop 1\n\tv_min_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf" : "+v"(s));
    asm volatile("s_nop 1\n\tv_min_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf" : "+v"(s));
    float up = __uint_as_float(0x7F800000u);
    asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(up) : "v"(s));
    return up;
}
struct WaveBall {  // wave-uniform: the live lanes' positions lie within rho of (px, py, pz)
    float px, py, pz, rho;
};
RM_DEV WaveBall wave_ball(float x, float y, float z, bool is_live, unsigned long long live_m) {
    WaveBall b;
    const int first = __builtin_ctzll(live_m);  // (the caller has a live lane)
    b.px = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(x), first));
    b.py = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(y), first));
    b.pz = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(z), first));
    const float dx = x - b.px, dy = y - b.py, dz = z - b.pz;
    const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
    // (non-negative floats order like their bit patterns; a NaN's pattern is above +inf's and wins: rho = NaN, nothing is far)
    const float r2 = __uint_as_float(wave_max_u32(is_live ? __float_as_uint(d2) : 0u));
    b.rho = __builtin_amdgcn_sqrtf(r2) * 1.00001f + 1.0e-30f;
    return b;
}
// The unit table in LDS (unit records are 32 bytes apart in device memory; a workgroup rearranges them when it stages the
// program), 8 n_units dwords in two parts:
//   dwords [0, 4 n_units)   one float4 per unit, RmDecoded::units[u].p[0..3]: centre and outer radius -- all a lattice mask asks
//                           of unit `lane`, so it is ONE 16-byte read per step (ds_read_b128 at lunits + 4 lane; a stride of 16
//                           bytes between lanes is what a 128-bit read serves without a conflict) where a row per field was four
//                           reads, four waits and four address registers live through the march loop;
//   rows 4 .. 7             one ROW of n_units dwords per field, at lunits + f n_units as before, so that lane u's reads do not
//                           collide with its neighbours': 4 inner radius, 5 blend radius, 6 kind; row 7 the record's first word
//                           (the records the unit stands for, first | last << 16).
// The table starts on a 16-byte boundary: behind the records (32 bytes each) behind the float4 cull tables; dynamic LDS itself.
constexpr uint32_t kUnitRows = 8u;
RM_DEV void stage_units(uint32_t* lunits, const RmRecord* __restrict__ units, uint32_t n_units, uint32_t tid, uint32_t n_threads) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(units);
    for (uint32_t k = tid; k < kUnitRows * n_units; k += n_threads) lunits[k] = src[rm_unit_table_source(k, n_units)];
}
// centre and outer radius of unit `lane` (unit 0 for the lanes at or above n_units)
RM_DEV float4 unit_sphere(const uint32_t* lunits, uint32_t n_units) {
    const uint32_t lane = threadIdx.x & 63u;
    return reinterpret_cast<const float4*>(lunits)[lane < n_units ? lane : 0u];
}
struct UnitBounds { float L, H, k; uint32_t kind; };
RM_DEV UnitBounds unit_bounds(const uint32_t* lunits, uint32_t n_units, const WaveBall& b) {
    const uint32_t lane = threadIdx.x & 63u;
    const float4 c = unit_sphere(lunits, n_units);
    const float* u = reinterpret_cast<const float*>(lunits) + (lane < n_units ? lane : 0u);
    const float dx = c.x - b.px, dy = c.y - b.py, dz = c.z - b.pz;
    const float d = __builtin_amdgcn_sqrtf(__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)));
    UnitBounds r;
    r.L = (d * 0.999998f - c.w) - b.rho;  // v_sqrt_f32 is within an ulp, the fused sum of squares within 3e-7
    r.H = (d * 1.000002f + b.rho) - u[4u * n_units];
    r.k = u[5u * n_units];
    r.kind = __float_as_uint(u[6u * n_units]);
    return r;
}
// (Measured and dropped: a mask good for TWO march steps -- a step moves a ray by at most thr and the next threshold is at most
// 2.0001 thr + m', so "|p* - c| - R - (rho + T) > 2.0001 T + m'" holds at both -- halves the cost of the masks and nearly
// doubles the leaves evaluated, 3.6 -> 6.8 of 16 per step on the metric scene: march kernel 0.544 -> 0.613 ms,
// profiles/r03_wave_level_culling_ab.txt.)
RM_DEV unsigned long long wave_cull_lattice(const uint32_t* lunits, uint32_t n_units, float x, float y, float z, float thr, bool is_live,
                                            unsigned long long live_m) {
    const unsigned long long valid = n_units >= 64u ? ~0ull : ((1ull << n_units) - 1ull);
    // ONE reduction: unit u is far for lane l when value_u(p_l) >= |p* - c| - R - |p_l - p*| > thr_l, i.e. for every live lane when
    // |p* - c| - R > S = max over live lanes (|p_l - p*| + thr_l) -- sharper than rho + T (a maximum of sums, not a sum of maxima)
    // and a wave reduction less.  thr >= 0 or NaN; a NaN's bit pattern is above +inf's and wins the maximum: nothing is far then.
    // (asked for first, and kept first: left to itself the scheduler issues the 128-bit read right in front of its use, behind the
    // reduction, and the step waits out the LDS latency the reduction would have covered)
    const float4 c = unit_sphere(lunits, n_units);
    __builtin_amdgcn_sched_barrier(0);
    const int first = __builtin_ctzll(live_m);  // (the caller has a live lane)
    const float px = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(x), first));
    const float py = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(y), first));
    const float pz = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(z), first));
    const float ex = x - px, ey = y - py, ez = z - pz;
    // The reach is taken in the L1 norm: |p_l - p*|_2 <= |p_l - p*|_1, so the triangle inequality holds a fortiori, and the sum
    // of three magnitudes is two additions (|.| is a source modifier) where the L2 norm is three multiply-adds and a v_sqrt_f32,
    // the one transcendental of a march step the arithmetic contract does not ask for (nothing overlaps one: DESIGN.md section 5).
    // The price is a larger S -- 3.63 leaves of 16 evaluated per step on the metric frame instead of 3.60 (tools/sim/wave_cull_sim.py;
    // 3.28 instead of 3.20 by the GPU's counters, profiles/r14_lattice_reach_ab.txt).
    // Slack, with u = 2^-24 (every operation below is rounded to nearest; a difference or a sum that lands among the denormals is
    // exact, and nothing is squared: no underflow, which is what the L2 form's "+ 1e-30f" was for -- ex * ex vanishes below 1e-19):
    //   x - px            a rounded difference is at least (1 - u) times the exact one:  |x - px| <= |ex| / (1 - u)
    //   the two additions a rounded sum is at least (1 - u) times the exact one:         |ex| + |ey| + |ez| <= l1 / (1 - u)^2
    //                     together |p_l - p*|_1 <= l1 / (1 - u)^3 < l1 (1 + 1.8e-7): the factor 1.00001f of the multiply-add covers it
    //                     fifty times over (the figure is the L2 form's, kept so that the two reaches differ by the norm alone);
    //   S * 1.000005f     the single rounding of the multiply-add (sl >= (1 - u) (l1 * 1.00001f + thr)), this product's own, and
    //                     the rounding of s = S + R below (thr >= 0 or NaN, R >= 0 or +inf: both are relative to a sum of non-negative
    //                     terms): 3 u = 1.8e-7 of 5e-6;
    //   1.000004f         on the squares, 2e-6 on the lengths: the three differences c - p* (u each), the three roundings of
    //                     the fused sum of their squares (d2 is below 1 + 3e-7 times the exact one), s * s and the product with
    //                     the constant (u each): 5e-7 of 4e-6 on the squares.
    // A NaN or an infinite coordinate, or a NaN or +inf threshold, of a live lane gives sl = +inf or NaN: both win the unsigned
    // maximum over every finite reach, S is not finite and no comparison below holds.  A dead lane passes 0, whatever it holds.
    const float l1 = (__builtin_fabsf(ex) + __builtin_fabsf(ey)) + __builtin_fabsf(ez);
    const float sl = __builtin_fmaf(l1, 1.00001f, thr);
    const float S = __uint_as_float(wave_max_u32(is_live ? __float_as_uint(sl) : 0u)) * 1.000005f;
    // far: |p* - c| - R > S, decided on the squares (every term is >= 0; a NaN or an infinity makes it false)
    const float dx = c.x - px, dy = c.y - py, dz = c.z - pz;
    const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
    const float s = S + c.w;
    return ~__builtin_amdgcn_ballot_w64(d2 > (s * s) * 1.000004f) & valid;
}
// margin_scale: scene_scale + |ro|_1 (the `prune_scale` of the kernels)
RM_DEV unsigned long long wave_cull_blend(const uint32_t* lunits, uint32_t n_units, float kmax, float x, float y, float z, float extra_margin,
                                          float margin_scale, bool is_live, unsigned long long live_m) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long valid = n_units >= 64u ? ~0ull : ((1ull << n_units) - 1ull);
    const WaveBall b = wave_ball(x, y, z, is_live, live_m);
    const float m = kPruneAbs * (margin_scale + ((__builtin_fabsf(b.px) + __builtin_fabsf(b.py)) + __builtin_fabsf(b.pz)) + 2.0f * b.rho) + extra_margin;
    const UnitBounds u = unit_bounds(lunits, n_units, b);
    const bool in_range = lane < n_units;
    const float inf = __uint_as_float(0x7F800000u);
    // (the lane predicates are combined with & and |, not && and ||: short-circuit evaluation of a lane predicate is divergent control
    // flow -- an exec mask saved, narrowed and restored per operator, a dozen scalar instructions where one s_and_b64 does)
    const bool blends = in_range & ((u.kind == RM_UNIT_UM) | (u.kind == RM_UNIT_START));
    const float a_hi = wave_exclusive_min(blends ? u.H : inf);
    const float a_lo = wave_exclusive_min(blends ? u.L : inf) - kmax;
    const bool is_um = u.kind == RM_UNIT_UM, is_sub = u.kind == RM_UNIT_SUB, is_int = u.kind == RM_UNIT_INTER;
    const bool far_um = u.L >= (a_hi + u.k) + m, far_sub = u.L + a_lo >= m, far_int = u.H <= a_lo - m;  // (false on a NaN)
    const bool skip = (is_um & far_um) | (is_sub & far_sub) | (is_int & far_int);
    const bool restart = is_um & (u.H <= (a_lo - u.k) - m);
    const unsigned long long opaque_m = __builtin_amdgcn_ballot_w64(u.kind == RM_UNIT_OPAQUE) & valid;
    const unsigned long long before_opaque = opaque_m ? ((1ull << __builtin_ctzll(opaque_m)) - 1ull) : ~0ull;
    const unsigned long long restart_m = __builtin_amdgcn_ballot_w64(restart) & valid & before_opaque;
    const unsigned long long skip_m = __builtin_amdgcn_ballot_w64(skip) & valid & before_opaque;
    const uint32_t r = restart_m ? 63u - (uint32_t)__builtin_clzll(restart_m) : 0u;
    const unsigned long long from_r = ~((1ull << r) - 1ull);  // units r .. 63
    // the first unit at or behind the restart that may have raised the accumulator, or behind which nothing is known
    const unsigned long long poison_m = (opaque_m | (__builtin_amdgcn_ballot_w64((is_sub | is_int) & !skip) & valid)) & from_r;
    const unsigned long long behind_poison = poison_m ? ~((2ull << __builtin_ctzll(poison_m)) - 1ull) : 0ull;  // (2 << 63 = 0: none)
    return valid & from_r & (~skip_m | behind_poison | (1ull << r));
}
// Tree programs under the interpreter (rm_interp.h map_scene_tree_masked): from the wave's unit mask to the RECORDS the wave has
// to execute.  Lane r looks at records r and r + 64 (RmDecoded::tree, staged like rows 4 .. 7 of the unit table: one row per field), L and R
// being the units of the record's operands:
//   a leaf is kept iff its unit is needed; an operator record iff both operands hold a needed leaf -- with one of them all +inf a
//   Union or the right side of a Subtraction is the identity on the other: dropped, with the operand's records;
//   a fused leaf whose left operand has gone (Union only, see below) pushes instead of combining: as_push;
//   a Subtraction whose LEFT operand has gone while the right one has not is max(+inf, .) = +inf only in name -- nothing would
//   push that +inf.  It FORCES the first leaf of its left operand back into the mask (evaluating a far leaf instead of replacing
//   it is always allowed).  One pass suffices: the forced leaf lies in an operand that was entirely empty, so no other
//   record's decision changes -- operators inside that operand still have an empty side, operators above it had a needed leaf on
//   this side already (the right operand's).
struct TreeKeep { unsigned long long keep0, keep1, push0, push1; };
RM_DEV TreeKeep tree_keep(const uint32_t* ltree, uint32_t n_rec, unsigned long long need) {
    const uint32_t lane = threadIdx.x & 63u;
    TreeKeep k{0ull, 0ull, 0ull, 0ull};
    const bool two = n_rec > 64u;  // wave-uniform
    unsigned long long Lm[2], Rm[2];
    uint32_t info[2];
    bool in[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const uint32_t r = lane + 64u * (uint32_t)h;
        in[h] = r < n_rec;
        const uint32_t* t = ltree + (in[h] ? r : 0u);
        if (h == 0 || two) {
            Lm[h] = (unsigned long long)t[0] | ((unsigned long long)t[n_rec] << 32);
            Rm[h] = (unsigned long long)t[2u * n_rec] | ((unsigned long long)t[3u * n_rec] << 32);
            info[h] = t[4u * n_rec];
        } else {
            Lm[h] = Rm[h] = 0ull;
            info[h] = 0u;
        }
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
        if (h == 1 && !two) break;
        unsigned long long fm = __builtin_amdgcn_ballot_w64(in[h] && rm_tree_forces(Lm[h], Rm[h], info[h], need));
        while (fm != 0ull) {  // rare
            const int l = __builtin_ctzll(fm);
            fm &= fm - 1ull;
            need |= 1ull << rm_tree_forced_unit((uint32_t)__builtin_amdgcn_readlane((int)info[h], l));
        }
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
        if (h == 1 && !two) break;
        const bool keep = in[h] && rm_tree_keeps(Lm[h], Rm[h], info[h], need);
        const unsigned long long km = __builtin_amdgcn_ballot_w64(keep), pm = __builtin_amdgcn_ballot_w64(keep && rm_tree_pushes(Lm[h], info[h], need));
        if (h == 0) { k.keep0 = km; k.push0 = pm; } else { k.keep1 = km; k.push1 = pm; }
    }
    return k;
}
RM_DEV void stage_tree(uint32_t* ltree, const RmRecord* __restrict__ tree, uint32_t n_tree, uint32_t tid, uint32_t n_threads) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(tree);
    for (uint32_t k = tid; k < 5u * n_tree; k += n_threads) {
        const uint32_t f = k / n_tree, r = k - f * n_tree;
        ltree[k] = src[8u * r + 1u + f];
    }
}
#undef RM_DPP

#if !defined(RM_JIT_TU)  // diagnostics (rm_selftest_wave)
__global__ __launch_bounds__(64) void rm_selftest_wave_kernel(const float* in, float* out, uint32_t n_waves) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const float x = in[i];
    out[i] = __uint_as_float(wave_max_u32(__float_as_uint(x)));
    out[64u * n_waves + i] = wave_exclusive_min(x);
}
#endif

// Is unit u (a compile-time constant in generated code) in the wave's mask.  The mask goes through an empty asm at every use:
// left alone the compiler computes all the tests where the mask is born and keeps sixteen 64-bit lane masks alive across the
// whole evaluation -- 30 more scalar registers spilled, which costs the vector register that decides between 6 and 5 waves
// per SIMD.  With the asm each test is born where it is used: s_bitcmp1_b64 + s_cbranch_scc.
RM_DEV bool unit_needed(unsigned long long need, uint32_t u) {
    // the half of the mask that holds the bit: s_mov_b32 + s_bitcmp1_b32
    uint32_t w = (uint32_t)(need >> (u & 32u));
    asm volatile("" : "+s"(w));
    return ((w >> (u & 31u)) & 1u) != 0u;
}

// A group of units behind one test (rm_jit.h): the 32-bit word of the mask that holds unit u, through the asm once for the group;
// the tests inside the group read it as it is (s_bitcmp1_b32)
RM_DEV uint32_t unit_word(unsigned long long need, uint32_t u) {
    uint32_t w = (uint32_t)(need >> (u & 32u));
    asm volatile("" : "+s"(w));
    return w;
}
RM_DEV bool unit_in_word(uint32_t w, uint32_t u) { return ((w >> (u & 31u)) & 1u) != 0u; }
// vmin(+inf, b) of the single-unit path (rm_jit.h "Single-unit steps"): the v_min_f32 a Union applies to a skipped (+inf) accumulator
// and the one leaf of the step, with +inf as a literal of the instruction -- as a register it is one more value live across the march
// loop of a kernel that sits at its register limit.  b for every number, +inf for a NaN.
RM_DEV float vmin_pinf(float b) {
    float r;
    asm("v_min_f32 %0, 0x7f800000, %1" : "=v"(r) : "v"(b));
    return r;
}

typedef float lds_f4 __attribute__((ext_vector_type(4)));
typedef float lds_f2 __attribute__((ext_vector_type(2)));
RM_DEV lds_f4 lds_load4(LdsF r) { return *reinterpret_cast<const __attribute__((address_space(3))) lds_f4*>(r); }
RM_DEV lds_f2 lds_load2(LdsF r) { return *reinterpret_cast<const __attribute__((address_space(3))) lds_f2*>(r); }
// Parameter reads of the generated code.  A specialised kernel stages every record ROTATED by one dword -- p[0..6] at
// dwords 0..6, the opcode (which generated code never reads) at dword 7 -- so that the parameters of a record start on
// a 32-byte boundary and are fetched with ONE ds_read_b128 (+ a ds_read_b64 for a box) instead of two or three
// ds_read2_b32: the LDS pipe of a CU serves a wave64 b32 / b64 read in 2 cycles and a read2_b32 / b128 in 4
// (MI355X_MICROARCH.md, LDS), it is shared by the four SIMDs, and at ~40 parameter reads per evaluation it was ~60 %
// busy (SQ_ACTIVE_INST_LDS) next to a vector unit at ~80 %.
RM_DEV float spec_sphere_a(LdsF r, float qx, float qy, float qz) {
    const lds_f4 p = lds_load4(r);  // cx cy cz r
    const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
    return (dx * dx + dy * dy) + dz * dz;  // the argument of sdf_sphere_t's sqrt, same operations
}
template <bool FAST>
RM_DEV float spec_sphere_v(LdsF r, float a, SqrtGuard& tiny) { return sqrt_sel<FAST>(a, tiny) - r[3]; }
// Subtracted leaves (mode SUB fused into the leaf): max(acc, -v) = acc whenever -v <= acc, in particular at every position
// OUTSIDE the leaf (v > 0) while acc >= 0.  Sphere: a > (r k)^2 (r k: RmRecord::p[4], k = 1.000005) puts sqrt(a) above r by
// more than its rounding, so the computed v = sqrt(a) - r is > 0; NaN fails the comparison and the leaf is evaluated.
RM_DEV bool spec_sub_sphere_near(unsigned long long live, LdsF r, float a, float acc) {
    const float rk = r[4];
    return ((__builtin_amdgcn_ballot_w64(!(a > rk * rk)) | __builtin_amdgcn_ballot_w64(!(acc >= 0.0f))) & live) != 0ull;
}
// Box: a = |max(q, 0)|^2 > 0 means some q_i > 0: the inside term is +0 and v = sqrt(a) > 0.
RM_DEV bool spec_sub_box_near(unsigned long long live, float a, float acc) {
    return ((__builtin_amdgcn_ballot_w64(!(a > 0.0f)) | __builtin_amdgcn_ballot_w64(!(acc >= 0.0f))) & live) != 0ull;
}
struct SpecBox { float qx, qy, qz, a; };
RM_DEV SpecBox spec_box_a(LdsF r, float px, float py, float pz) {
    const lds_f4 c = lds_load4(r);       // cx cy cz rx
    const lds_f2 h = lds_load2(r + 4);   // ry rz
    SpecBox b;
    b.qx = __builtin_fabsf(px - c.x) - c.w;
    b.qy = __builtin_fabsf(py - c.y) - h.x;
    b.qz = __builtin_fabsf(pz - c.z) - h.y;
    const float mx = fmax_(b.qx, 0.0f), my = fmax_(b.qy, 0.0f), mz = fmax_(b.qz, 0.0f);
    b.a = (mx * mx + my * my) + mz * mz;  // as sdf_box_t
    return b;
}
template <bool FAST>
RM_DEV float spec_box_v(const SpecBox& b, SqrtGuard& tiny) {
    return sqrt_sel<FAST, true, kBoxGuardLo>(b.a, tiny) + fmin_(fmax_(b.qx, fmax_(b.qy, b.qz)), 0.0f);
}
// Leaves and the one operator with a parameter, as the generated code calls them: `r` points at the
// record's parameters in LDS (wave-uniform address, constant offset: a broadcast read).  A box guards the lower
// side of its root only where the kernel still has to (kBoxGuardLo: rm_interp.h "Range proofs").
template <bool FAST>
RM_DEV float spec_sphere(LdsF r, float qx, float qy, float qz, SqrtGuard& tiny) {
    const lds_f4 c = lds_load4(r);
    const float p[7] = {c.x, c.y, c.z, c.w, 0.0f, 0.0f, 0.0f};
    return sdf_sphere_t<FAST>(qx, qy, qz, p, tiny);
}
template <bool FAST>
RM_DEV float spec_box(LdsF r, float qx, float qy, float qz, SqrtGuard& tiny) {
    const lds_f4 c = lds_load4(r);
    const lds_f2 h = lds_load2(r + 4);
    const float p[7] = {c.x, c.y, c.z, c.w, h.x, h.y, 0.0f};
    return sdf_box_t<FAST, kBoxGuardLo>(qx, qy, qz, p, tiny);
}
template <bool FAST>
RM_DEV float spec_cylinder(LdsF r, float qx, float qy, float qz, SqrtGuard& tiny) {
    const lds_f4 c = lds_load4(r);
    const float p[7] = {c.x, c.y, c.z, c.w, r[4], 0.0f, 0.0f};
    return sdf_cylinder_t<FAST>(qx, qy, qz, p, tiny);
}
RM_DEV float spec_plane(LdsF r, float qx, float qy, float qz) {
    const lds_f4 n = lds_load4(r);
    return ((qx * n.x + qy * n.y) + qz * n.z) + n.w;  // as exec_command
}
// k of a SmoothUnion record as a SCALAR: every lane reads the same LDS word, but the compiler cannot know, and "if (k > 0)" on a vector
// register is divergent control flow (exec saved, narrowed, restored: a dozen scalar instructions per blend, at 4.3 cycles each)
RM_DEV float uniform_k(LdsF r) { return __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(r[0]))); }
RM_DEV float spec_smooth_union(LdsF r, float a, float b, unsigned long long live) {  // as exec_command, RM_MODE_SMOOTH
    const float kk = uniform_k(r);
    float v = fmin_(a, b);
    if (kk > 0.0f) {
        const float t = kk - __builtin_fabsf(a - b);
        // Outside the blend zone (t <= 0, or NaN) h is 0 and, k being finite, the result is v - 0 = v exactly.  When
        // that holds for every live lane of the wave -- most evaluations: two operands are within k of each other
        // only near the seams -- the division and the five operations after it are skipped (dead lanes' values are
        // never used).
        if (kk < __uint_as_float(0x7F800000u) && (__builtin_amdgcn_ballot_w64(t > 0.0f) & live) == 0ull) return v;
        const float h = fmax_(t, 0.0f) / kk;
        v = v - ((h * h) * kk) * 0.25f;
    }
    return v;
}

// Pins the running minimum / maximum of a SqrtGuard at this point of the generated code.  The guard folds the bit pattern
// of every sqrt argument of an evaluation into two integers; integer min / max may be reassociated, and the compiler
// rebuilt the sequential updates of the four-tap function (64 arguments for a 16-leaf program) into trees that combine
// the FIRST arguments LAST -- every argument stayed live to the end: +55 VGPRs, the difference between 6 and 3-4 waves
// per SIMD for the smooth-min and material scenes (round 1 blamed the four copies of SmoothUnion's division and kept such
// programs on one-position taps).  Measured on the smooth-min scene at 4K: 15.6 ms without the fence, 11.6 ms with it.
RM_DEV void guard_fence(SqrtGuard& g) { asm("" : "+v"(g.lo), "+v"(g.hi)); }

// The same operator applied to the four tap values of a hit (map_scene_taps): ONE wave-uniform "is any live lane of any
// tap inside the blend zone" test for the four.  A lane outside the zone has h = 0 and gets v - 0 = v: the value the
// skipping form returns.
RM_DEV void spec_smooth_union4(LdsF r, const float (&a)[4], const float (&b)[4], unsigned long long live, float (&out)[4]) {
    const float kk = uniform_k(r);
    float t[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        out[i] = fmin_(a[i], b[i]);
        t[i] = kk - __builtin_fabsf(a[i] - b[i]);
    }
    if (!(kk > 0.0f)) return;
    const unsigned long long in_zone = (__builtin_amdgcn_ballot_w64(t[0] > 0.0f) | __builtin_amdgcn_ballot_w64(t[1] > 0.0f)) |
                                       (__builtin_amdgcn_ballot_w64(t[2] > 0.0f) | __builtin_amdgcn_ballot_w64(t[3] > 0.0f));
    if (kk < __uint_as_float(0x7F800000u) && (in_zone & live) == 0ull) return;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float h = fmax_(t[i], 0.0f) / kk;
        out[i] = out[i] - ((h * h) * kk) * 0.25f;
        __builtin_amdgcn_sched_barrier(0);  // one correctly rounded division in flight: interleaved, the four need ~60 more VGPRs
    }
}

// sizes of a march wave's ready / miss / hit buffers and of the tile's ray pool: rm_lds_layout.h
using rml::V5_RQ; using rml::V5_SQ; using rml::V5_HQ; using rml::V5_POOL;
// typed pointer to a byte offset of the workgroup's dynamic LDS (offsets: the layouts of rm_lds_layout.h)
template <class T>
RM_DEV T* lds_at(uint32_t* smem, uint32_t byte_offset) { return reinterpret_cast<T*>(reinterpret_cast<char*>(smem) + byte_offset); }

// Miss-test tables of a program, built per workgroup in LDS from the decoded records (the
// decoder stores each primitive's slot within its kind in RmRecord::p[6]):
//   cone[n_cone]  one float4 per sphere: (m.x, m.y, m.z, s); a ray clears it iff m.d - s < 0
//   slab[n_slab]  three float4 per box / cylinder: lo - o and hi - o of the bounding box inflated by
//                 the margin, then the cone of that box's bounding sphere (a cheap pre-test: only
//                 if some lane's ray enters that cone does the wave run the 6-multiply slab test)
//   veto          bit 0: something is non-finite, nothing may be culled; bit 1: the program has a Plane, the tables cannot
//                 clear a ray (the miss test on lower bounds still can)
struct CullTables {
    const float4* cone;
    const float4* slab;
    const uint32_t* veto;
    uint32_t n_cone, n_slab;
};

// Scale of the coordinates a ray from `ro` meets: what the margins of "Pruning" are multiples of ...
RM_DEV float prune_scale_v5(const RmLaunch& L, const V4& ro) {
    return L.scene_scale + ((__builtin_fabsf(ro.x) + __builtin_fabsf(ro.y)) + __builtin_fabsf(ro.z));
}
// ... and, with the blends' slack, what the bounds of "Miss test on lower bounds" are computed from.  The three terms are added
// up in two orders, which round differently: the march kernel (and the self-test of its ray test) starts from its prune_scale,
// the pre-pass (and the self-test of its pixel test) from the program's two terms.  Each verdict is pinned with its own sum.
RM_DEV float bound_scale_march_v5(const RmLaunch& L, const V4& ro) { return prune_scale_v5(L, ro) + L.smooth_slack; }
RM_DEV float bound_scale_prepass_v5(const RmLaunch& L, const V4& ro) {
    return (L.scene_scale + L.smooth_slack) + ((__builtin_fabsf(ro.x) + __builtin_fabsf(ro.y)) + __builtin_fabsf(ro.z));
}

// `slack`: how far SmoothUnion operators can pull the tree value below the minimum over its leaves
// (each lowers min(a,b) by at most k/4; nested operators add up).  0 for reference-only programs.
RM_DEV float cull_margin(float cx, float cy, float cz, float rho, const V4& ro, float min_dist, float slack) {
    const float scale = 1.0f + __builtin_fabsf(cx) + __builtin_fabsf(cy) + __builtin_fabsf(cz) + rho +
                        __builtin_fabsf(ro.x) + __builtin_fabsf(ro.y) + __builtin_fabsf(ro.z) + slack;
    return (fmax_(min_dist, 0.0f) + slack) * 1.01f + 1.0e-4f * scale;
}

// Table entry (or entries) of one record; no-op for operators.  Called once per record per workgroup.
RM_DEV void cull_build_v5(const RmRecord& rec, const V4& ro, float min_dist, float slack, float4* cone, float4* slab,
                          uint32_t* veto, const float4* bounds = nullptr) {
    uint32_t kind = RM_OP_KIND(rec.op);
    if (kind == RM_KIND_POP || kind == RM_KIND_XFORM) return;
    if (rec.op & RM_OP_NOCULL) {  // subtracted: a hit needs the left operand's surface, whatever this one does
        // (a program with transforms keeps a cone slot per bounded primitive: this one's clears every ray and every pixel)
        if (bounds && kind != RM_KIND_PLANE) cone[__float_as_uint(rec.p[6])] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
        return;
    }
    if (kind == RM_KIND_PLANE) { atomicOr(veto, 2u); return; }  // unbounded primitive: the tables cannot clear anything (bit 1)
    const float inf = __uint_as_float(0x7F800000u);
    const uint32_t slot = __float_as_uint(rec.p[6]);
    float cx = rec.p[0], cy = rec.p[1], cz = rec.p[2], sphere_r = rec.p[3];
    if (bounds) {  // program with transforms: the host computed a world-space bounding sphere for every bounded primitive
        const float4 b = bounds[slot];
        cx = b.x; cy = b.y; cz = b.z; sphere_r = b.w;
        kind = RM_KIND_SPHERE;
    }
    bool finite = __builtin_fabsf(cx) < inf && __builtin_fabsf(cy) < inf && __builtin_fabsf(cz) < inf &&
                  __builtin_fabsf(ro.x) < inf && __builtin_fabsf(ro.y) < inf && __builtin_fabsf(ro.z) < inf &&
                  __builtin_fabsf(min_dist) < inf;
    if (kind == RM_KIND_SPHERE) {
        const float rho = fmax_(sphere_r, 0.0f);
        finite = finite && rho < inf;
        const float Rk = rho + cull_margin(cx, cy, cz, rho, ro, min_dist, slack);
        const float mx = cx - ro.x, my = cy - ro.y, mz = cz - ro.z;
        const float mm = mx * mx + my * my + mz * mz;
        // s < sqrt(|m|^2 - Rk^2), the slack covering the rounding of this computation and of the
        // per-ray dot product (|error| <= ~4e-7 |m|)
        const float lim = mm * (1.0f - 4.0e-6f) - Rk * Rk * (1.0f + 4.0e-6f);
        float sv = -inf;  // origin inside (or not clearly outside) the inflated sphere: never clear
        if (lim > 0.0f && lim < inf) sv = __builtin_sqrtf(lim) * (1.0f - 1.0e-5f) - 1.0e-5f * __builtin_sqrtf(mm);
        cone[slot] = make_float4(mx, my, mz, sv);
    } else {
        // box: half extents; cylinder (extension): its bounding box (radius, half height, radius)
        const bool cyl = kind == RM_KIND_CYLINDER;
        const float hx = fmax_(rec.p[3], 0.0f), hy = fmax_(rec.p[4], 0.0f), hz = cyl ? hx : fmax_(rec.p[5], 0.0f);
        finite = finite && hx < inf && hy < inf && hz < inf;
        const float M = cull_margin(cx, cy, cz, hx + hy + hz, ro, min_dist, slack);
        slab[3u * slot] = make_float4((cx - hx - M) - ro.x, (cy - hy - M) - ro.y, (cz - hz - M) - ro.z, 0.0f);
        slab[3u * slot + 1u] = make_float4((cx + hx + M) - ro.x, (cy + hy + M) - ro.y, (cz + hz + M) - ro.z, 0.0f);
        // bounding-sphere cone of the inflated box (same construction as for spheres)
        const float Rk = __builtin_sqrtf((hx + M) * (hx + M) + (hy + M) * (hy + M) + (hz + M) * (hz + M)) * (1.0f + 1.0e-5f);
        const float mx = cx - ro.x, my = cy - ro.y, mz = cz - ro.z;
        const float mm = mx * mx + my * my + mz * mz;
        const float lim = mm * (1.0f - 4.0e-6f) - Rk * Rk * (1.0f + 4.0e-6f);
        float sv = -inf;  // origin not clearly outside the bounding sphere: always run the slab test
        if (lim > 0.0f && lim < inf) sv = __builtin_sqrtf(lim) * (1.0f - 1.0e-5f) - 1.0e-5f * __builtin_sqrtf(mm);
        slab[3u * slot + 2u] = make_float4(mx, my, mz, sv);
    }
    if (!finite || !(slack < inf)) atomicOr(veto, 1u);  // bit 0: non-finite data, nothing may be culled by any test
}

// Per-tile primitive mask (the pre-pass's tile_touch_mask_v5 makes it, one word per tile): bit k set for cone entry k, bit
// n_cone + k for slab entry k, iff the tile's cone does not provably clear that entry -- the tile test has proven that every
// sample ray of the tile clears each entry whose bit is 0, so a ray or a pixel of the tile tests the set bits only.  All ones:
// nothing is known about the tile (more than 32 entries, tables or cone unusable, rows not consecutive) and every entry is tested,
// by the loops over the whole tables.  A mask in use belongs to a program of at most 32 entries and never has a bit at or above
// n_cone + n_slab, so it is never all ones unless all 32 entries are touched -- and then both ways test the same entries.
// (Walking the set bits with s_ff1 costs nothing per cleared entry; a bit test per entry inside the old loops gave +0.6 % of
// headline where this form gives +2 %: profiles/r16_tile_masks_ab.txt.)
constexpr uint32_t V5_MASK_ALL = 0xFFFFFFFFu;
// the cone / slab bits of a mask in use (n_cone + n_slab <= 32)
RM_DEV uint32_t mask_cone_bits(uint32_t mask, uint32_t n_cone) { return n_cone >= 32u ? mask : mask & ((1u << n_cone) - 1u); }
RM_DEV uint32_t mask_slab_bits(uint32_t mask, uint32_t n_cone) { return n_cone >= 32u ? 0u : mask >> n_cone; }

// One entry of the ray test.  Cone k: the ray clears it iff m.d - s < 0 (NaN -> not clear).
RM_DEV void ray_cone_entry_v5(const CullTables& T, uint32_t k, float dx, float dy, float dz, bool& clear) {
    const float4 a = T.cone[k];  // wave-uniform address: LDS broadcast
    const float t = __builtin_fmaf(a.z, dz, __builtin_fmaf(a.y, dy, __builtin_fmaf(a.x, dx, -a.w)));
    clear = clear && (t < 0.0f);
}
// Slab k, (ix, iy, iz) = 1 / d; returns true when no lane of the wave is clear any more.
RM_DEV bool ray_slab_entry_v5(const CullTables& T, uint32_t k, float dx, float dy, float dz, float ix, float iy, float iz, bool& clear) {
    const float4 c = T.slab[3u * k + 2u];
    const float t = __builtin_fmaf(c.z, dz, __builtin_fmaf(c.y, dy, __builtin_fmaf(c.x, dx, -c.w)));
    if (__ballot(clear && !(t < 0.0f)) == 0ull) return false;  // every still-clear ray misses the bounding sphere
    const float4 a = T.slab[3u * k], b = T.slab[3u * k + 1u];
    const float x1 = a.x * ix, x2 = b.x * ix, y1 = a.y * iy, y2 = b.y * iy, z1 = a.z * iz, z2 = b.z * iz;
    const float tn = fmax_(fmin_(x1, x2), fmax_(fmin_(y1, y2), fmin_(z1, z2)));
    const float tf = fmin_(fmax_(x1, x2), fmin_(fmax_(y1, y2), fmax_(z1, z2)));
    clear = clear && !(tf >= fmax_(tn, 0.0f));  // a dropped NaN only widens the interval
    return __ballot(clear) == 0ull;
}
// 1/d with |d_i| clamped away from 0 so that no 0 * inf = NaN can appear in the slab test
RM_DEV float slab_rcp_v5(float d) { return __builtin_amdgcn_rcpf(__builtin_copysignf(fmax_(__builtin_fabsf(d), 1.0e-30f), d)); }

// true iff the half-line o + t d (t >= 0) provably stays clear of every primitive's margin zone.  mask (wave-uniform): the
// primitive mask of the ray's tile, V5_MASK_ALL for a ray of no tile.
RM_DEV bool ray_misses_scene_v5(const CullTables& T, uint32_t mask, float dx, float dy, float dz) {
    bool clear = *T.veto == 0u;  // no primitives (empty scene): every ray misses (wgsl:189-191)
    unit_dir(dx, dy, dz);        // the tests are about the half-line, whatever the length of d (see unit_dir)
    if (mask != V5_MASK_ALL) {  // a mask in use (at most 32 entries): its set bits in ascending order, 1.7 of 13 on the metric frame
        for (uint32_t m = mask_cone_bits(mask, T.n_cone); m != 0u; m &= m - 1u) ray_cone_entry_v5(T, (uint32_t)__builtin_ctz(m), dx, dy, dz, clear);
        const uint32_t ms = mask_slab_bits(mask, T.n_cone);
        if (ms == 0u || __ballot(clear) == 0ull) return clear;
        const float ix = slab_rcp_v5(dx), iy = slab_rcp_v5(dy), iz = slab_rcp_v5(dz);
        for (uint32_t m = ms; m != 0u; m &= m - 1u)
            if (ray_slab_entry_v5(T, (uint32_t)__builtin_ctz(m), dx, dy, dz, ix, iy, iz, clear)) return false;
        return clear;
    }
    for (uint32_t k = 0; k < T.n_cone; k++) {
        ray_cone_entry_v5(T, k, dx, dy, dz, clear);
        if ((k & 3u) == 3u && __ballot(clear) == 0ull) return false;
    }
    if (T.n_slab == 0u || __ballot(clear) == 0ull) return clear;
    const float ix = slab_rcp_v5(dx), iy = slab_rcp_v5(dy), iz = slab_rcp_v5(dz);
    for (uint32_t k = 0; k < T.n_slab; k++)
        if (ray_slab_entry_v5(T, k, dx, dy, dz, ix, iy, iz, clear)) return false;
    return clear;
}

// ---- Miss test on lower bounds (programs with SmoothUnion; RmDecoded::bound_walk) -------------------------------
// The plain tests clear a ray when it stays farther than the margin from EVERY primitive, and for a program that blends
// the margin carries the blend's reach (RmDecoded::smooth_slack, = k for a chain of SmoothUnion(k)): a ray that passes one
// primitive at 0.1 is marched although nothing else is within 0.5 of it and the tree value never drops below 0.1 there.
// Sharper, and still exact: every operator admitted here is monotone non-decreasing in each operand --
//     min(a, b), max(a, b), smin_k(a, b) = min(a, b) - h^2 k / 4 with h = max(k - |a - b|, 0) / k  (d/da, d/db in [0, 1])
// -- except the right operand of a Subtraction, and max(a, -b) >= a.  So with c_i <= v_i(q) for every position q of the
// half-line (c_i: how close the half-line comes to leaf i), running the PROGRAM on the c_i -- Subtraction keeping its left
// operand -- gives L <= F(q) for every q of the half-line: if L exceeds the hit threshold (plus the same float slack as the
// plain tests), no march position of the ray can register a hit (wgsl:97), whatever the steps, and the ray is shaded as
// a miss.  Bounds along the half-line o + t d, |d| = 1, t >= 0:
//     sphere  |q - c| - r >= dist(half-line, c) - r                     (exact: |m x d| if m.d > 0, else |m|)
//     box     sdf_box >= Chebyshev distance to the box [c - h+, c + h+], h+ = max(h, 0): the smallest inflation delta at
//             which the slab intervals [tn_i - delta / |d_i|, tf_i + delta / |d_i|] and t >= 0 have a common point, i.e.
//             max over i != j of (tn_i - tf_j) / (1 / |d_i| + 1 / |d_j|) and over j of -tf_j |d_j|
// All of it may use fused multiply-adds and approximate reciprocals: these are bounds, not values of the arithmetic
// contract; every bound is lowered by 1e-5 of itself plus 2e-6 of the scene's scale, NaN becomes -3e38 (v_max drops a NaN
// operand, a min over bounds must not).  Runs only for the rays the plain tests could not clear.
// CONE (the pre-pass): (dx, dy, dz) is the unit centre direction of a pixel whose sixteen sample directions e all satisfy
// |e - c| <= rho.  The point at distance t on such a ray is within t rho of the centre ray's, leaves are 1-Lipschitz, and
// beyond T = |m| + R + max(c_i, 0) a leaf of bounding radius R around m is farther than max(c_i, 0) anyway, so
//     c_i(pixel) >= c_i(centre ray) - rho (|m| + R + max(c_i, 0)),
// the same inflation the plain pixel test applies to its cones and slabs.
// ray_bound_v5: the bound L itself (the self-test rm_selftest_cull_rays reads it); ray_misses_by_bounds_v5: the verdict.
template <bool CONE, class LoadRecord>
RM_DEV float ray_bound_v5(const LoadRecord& load, uint32_t n_rec, const V4& ro, float dx, float dy, float dz, float scale, float rho = 0.0f) {
    if (!CONE) unit_dir(dx, dy, dz);
    const float tiny = 1.0e-18f;  // |d_i| is clamped away from 0: 1 / |d_i| times a coordinate (< 1e12, RmDecoded::bound_walk) stays finite
    const float ax = fmax_(__builtin_fabsf(dx), tiny), ay = fmax_(__builtin_fabsf(dy), tiny), az = fmax_(__builtin_fabsf(dz), tiny);
    const float ix = __builtin_amdgcn_rcpf(__builtin_copysignf(ax, dx)), iy = __builtin_amdgcn_rcpf(__builtin_copysignf(ay, dy));
    const float iz = __builtin_amdgcn_rcpf(__builtin_copysignf(az, dz));
    const float wxy = (ax * ay) * __builtin_amdgcn_rcpf(ax + ay), wxz = (ax * az) * __builtin_amdgcn_rcpf(ax + az);
    const float wyz = (ay * az) * __builtin_amdgcn_rcpf(ay + az);
    const float lower = 2.0e-6f * scale;
    const float inf = __uint_as_float(0x7F800000u);
    float acc = inf, spilled = inf;
    for (uint32_t i = 0u; i < n_rec; i++) {
        uint32_t op;
        float p[7];
        load(i, op, p);
        op = __builtin_amdgcn_readfirstlane(op);
        const uint32_t kind = RM_OP_KIND(op), mode = RM_OP_MODE(op);
        float a, b;
        if (kind == RM_KIND_POP) {
            a = spilled; b = acc;
        } else {
            const float mx = p[0] - ro.x, my = p[1] - ro.y, mz = p[2] - ro.z;
            const float mm = __builtin_fmaf(mz, mz, __builtin_fmaf(my, my, mx * mx));
            float reach = 0.0f;  // CONE: bounding radius of the leaf
            bool bounded = true;
            if (kind == RM_KIND_PLANE) {
                // dot(q, n) + h is linear along a ray: v0 + t (n.d); over t >= 0 its infimum is v0 when n.d >= 0, else -inf.
                // CONE: every sample direction e has n.e >= n.c - |n| rho.  |n| is arbitrary (the value is not a distance): the
                // slack scales with it.
                const float nn = __builtin_amdgcn_sqrtf(__builtin_fmaf(p[2], p[2], __builtin_fmaf(p[1], p[1], p[0] * p[0]))) * 1.00001f;
                const float v0 = __builtin_fmaf(p[2], ro.z, __builtin_fmaf(p[1], ro.y, p[0] * ro.x)) + p[3];
                const float nd = __builtin_fmaf(p[2], dz, __builtin_fmaf(p[1], dy, p[0] * dx));
                const float slope = CONE ? nd - nn * (rho * 1.00001f) : nd;
                const float away = 1.0e-5f * nn;  // covers the rounding of n.d and of the march positions' own n.q
                b = slope >= away ? v0 - (1.0e-5f * (__builtin_fabsf(v0) + __builtin_fabsf(p[3])) + nn * (4.0f * lower)) : -inf;
                bounded = false;
            } else if (kind == RM_KIND_SPHERE) {
                const float cx = __builtin_fmaf(my, dz, -(mz * dy)), cy = __builtin_fmaf(mz, dx, -(mx * dz)), cz = __builtin_fmaf(mx, dy, -(my * dx));
                const float perp2 = __builtin_fmaf(cz, cz, __builtin_fmaf(cy, cy, cx * cx));
                reach = fmax_(p[3], 0.0f);
                const float along = __builtin_fmaf(mz, dz, __builtin_fmaf(my, dy, mx * dx));
                const float dist = __builtin_amdgcn_sqrtf(along > 0.0f ? perp2 : mm);
                b = dist * (1.0f - 1.0e-5f) - p[3];
            } else {  // RM_KIND_BOX; RM_KIND_CYLINDER through its bounding box (radius, half height, radius): a solid inside
                      // another is at least as far as that one
                const bool cyl = kind == RM_KIND_CYLINDER;
                const float hx = fmax_(p[3], 0.0f), hy = fmax_(p[4], 0.0f), hz = cyl ? hx : fmax_(p[5], 0.0f);
                reach = (hx + hy) + hz;  // >= |h|
                const float x1 = (mx - hx) * ix, x2 = (mx + hx) * ix, y1 = (my - hy) * iy, y2 = (my + hy) * iy;
                const float z1 = (mz - hz) * iz, z2 = (mz + hz) * iz;
                const float nx = fmin_(x1, x2), fx = fmax_(x1, x2), ny = fmin_(y1, y2), fy = fmax_(y1, y2);
                const float nz = fmin_(z1, z2), fz = fmax_(z1, z2);
                const float d0 = fmax_((nx - fy) * wxy, (ny - fx) * wxy);
                const float d1 = fmax_((nx - fz) * wxz, (nz - fx) * wxz);
                const float d2 = fmax_((ny - fz) * wyz, (nz - fy) * wyz);
                const float d3 = fmax_(-fx * ax, fmax_(-fy * ay, -fz * az));
                // (every product is finite: coordinates < 1e12 -- the caller checks the scale -- times 1 / |d_i| <= 1e18; a NaN
                // term dropped by v_max could only lower the maximum)
                const float delta = fmax_(fmax_(d0, d1), fmax_(d2, d3));
                b = delta * (1.0f - 1.0e-5f);
            }
            if (CONE && bounded) b = b - (rho * 1.00001f) * ((__builtin_amdgcn_sqrtf(mm) * 1.00001f + reach) + fmax_(b, 0.0f));
            b = fmax_(b - (lower + 1.0e-5f * __builtin_fabsf(b)), -3.0e38f);  // NaN -> -3e38
            if (op & RM_OP_SPILL) spilled = acc;
            a = acc;
        }
        if (mode == RM_MODE_PUSH) acc = b;
        else if (mode == RM_MODE_UNION) acc = fmin_(a, b);
        else if (mode == RM_MODE_SUB) acc = a;                      // max(a, -b) >= a
        else if (mode == RM_MODE_INTER) acc = fmax_(a, b);
        else {  // RM_MODE_SMOOTH
            const float kk = p[0];
            float v = fmin_(a, b);
            if (kk > 0.0f) {
                const float h = fmax_(kk - __builtin_fabsf(a - b), 0.0f) * __builtin_amdgcn_rcpf(kk);
                v = v - ((h * h) * kk) * 0.25f;
                v = v - (1.0e-6f * (__builtin_fabsf(v) + kk));
            }
            acc = fmax_(v, -3.0e38f);  // NaN (k = inf) -> -3e38
        }
    }
    return acc;
}
template <bool CONE, class LoadRecord>
RM_DEV bool ray_misses_by_bounds_v5(const LoadRecord& load, uint32_t n_rec, const V4& ro, float dx, float dy, float dz, float min_dist,
                                    float scale, float rho = 0.0f) {
    const float acc = ray_bound_v5<CONE>(load, n_rec, ro, dx, dy, dz, scale, rho);
    const float margin = fmax_(min_dist, 0.0f) * 1.01f + 1.0e-4f * scale;
    return acc > margin;  // NaN -> false
}

// Work list produced by the pre-pass (rm_tile_pre_v5 + rm_tile_sort_v5), one per frame.
struct V5Work {
    const uint32_t* order;  // [n_frames][n_tiles] ids of the tiles that need marching, heaviest first
    uint32_t* counters;     // [n_frames][4]: {number of such tiles, cursor of the persistent workgroups,
                            //                 bits of f0 = map_scene(ro) (the shared first march step), unused}
    uint32_t* measured;     // nullptr, or [n_frames][n_tiles]: how long each marched tile took (10 ns ticks), written here
                            // and read by the NEXT draw's rm_tile_sort_v5 (RM_OPT_BALANCE = 3: longest tiles first)
    const uint32_t* masks;  // [n_frames][n_tiles] primitive mask of every tile (rm_tile_pre_v5; V5_MASK_ALL: nothing known)
};

// (Round 3 tried to drop the sort kernel -- the pre-pass appending every tile that needs marching to one of four lists by the
// class of its last duration, one atomic per tile, the march kernel walking the classes: the frame's ~7 500 returning atomics
// on four addresses took the pre-pass from 0.06 to 0.21 ms, and four classes order the tiles worse than the sort's 64 buckets
// (8-node scene: march kernel 0.244 -> 0.277 ms).  How much the order is worth: last frame's durations 0.532 ms, pending
// pixels 0.65, order of arrival 0.66 on the metric frame.  profiles/r03_work_list_by_atomics_negative.txt)
// b for the lanes whose bit is set in the wave mask m, a for the others: one v_cndmask_b32 with the mask as its
// scalar operand.
RM_DEV float select_by_mask(float a, float b, unsigned long long m) {
    float r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(m));
    return r;
}
RM_DEV uint32_t select_by_mask(uint32_t a, uint32_t b, unsigned long long m) {
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(m));
    return r;
}
// this lane's bit of a wave mask as a predicate
RM_DEV bool lane_of(unsigned long long m, uint32_t lane) {
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(r) : "s"(m));
    (void)lane;
    return r != 0u;
}

struct TrueTag { static constexpr bool value = true; };
struct FalseTag { static constexpr bool value = false; };

// Persistent workgroups: the grid holds about as many workgroups as the chip has room for; each
// takes the next tile of the work list with one atomic and leaves when the list is exhausted
// (no spinning, no inter-workgroup dependency).  Tiles whose 1024 rays are all culled never reach
// this kernel: the pre-pass writes their pixels directly.
// MAT (extension, materials): compiled into the kernels that can meet a tagged program -- the extension
// interpreter and the kernels specialised for one; it adds a fifth phase after the four normal taps of a batch of
// hits (one evaluation of the material program at the hit positions) and a byte per ray next to its result code.
// LOOP (interpreter kernels): 0 the record loop is chosen at run time from the launch's flags; 1 chain, 2 chain over the records the unit
// mask names, 3 tree, 4 tree over the records the mask leaves -- a kernel compiled for ONE loop: no dispatch per evaluation, and above
// all none of the other loops' code and registers (the lean kernel with all four kept 176 scalar registers spilled in vector lanes)
template <class Prog, bool PROG_IN_LDS, int WPT, bool EXT, bool SPEC, bool MAT = false, int LOOP = 0>
RM_DEV void rm_render_v5_body(const RmLaunch& L, const V5Work& work, uint32_t n_tiles, uint32_t refill_min) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    // ---- LDS carve-up: rml::MarchLds (rm_lds_layout.h), from which the launch is sized.  Everything fixed at compile time is
    // taken from it; the offsets that depend on the launch are the same sums, written out on L's fields: through the
    // layout object (by value, inlined) the tree interpreters and the scalar-cache kernels came out with one or two more
    // scalar registers spilled (profiles/r15_lds_layout_kernel_resources.txt).  tests/cpp/lds_layout_check.cpp holds these sums
    // against the layout over every size a launch can have. ----
    typedef rml::MarchWaveLds WL;
    float* res = reinterpret_cast<float*>(smem);                       // [V5_POOL] result code per ray (tile)
    uint32_t* wbase = smem + V5_POOL + wave * L.wave_dwords;           // this wave's buffers
    uint32_t* rq_rid = wbase + WL::rq_rid / 4u;                        // ready rays (SoA): id, direction
    float* rq_d = reinterpret_cast<float*>(wbase + WL::rq_d / 4u);     // [3][V5_RQ]
    uint32_t* sq_rid = wbase + WL::sq_rid / 4u;                        // rays that ended without a hit: id, direction
    float* sq_v = reinterpret_cast<float*>(wbase + WL::sq_v / 4u);     // [3][V5_SQ]
    uint32_t* hq_rid = wbase + WL::hq_rid / 4u;                        // hits waiting for their normal: id, position
    float* hq_v = reinterpret_cast<float*>(wbase + WL::hq_v / 4u);     // [3][V5_HQ]
    float* wxy = reinterpret_cast<float*>(wbase + WL::wxy / 4u);       // [16] pt_screen.x of the tile's 8 columns, .y of its 8 rows (wgsl:41-43)
    float* tn = reinterpret_cast<float*>(wbase + WL::tn / 4u);         // [3][64] partial normals of the running tap phase (absent when L.wave_dwords says so)
    uint32_t* after = smem + V5_POOL + WPT * L.wave_dwords;            // MarchLds::spill
    float* spill = reinterpret_cast<float*>(after) + wave * (L.spill_depth * 64u) + lane;  // [WPT][depth][64]
    float4* t_cone = reinterpret_cast<float4*>(after + WPT * L.spill_depth * 64u);         // [n_cone]
    float4* t_slab = t_cone + L.n_cone;                                                     // [3 * n_slab]
    uint32_t* lprog = reinterpret_cast<uint32_t*>(t_slab + 3u * L.n_slab);                  // PROG_IN_LDS: records, unit table, tree table
    uint32_t* s_next = lprog + (PROG_IN_LDS ? (L.n_rec + L.n_grp + L.n_tree) * 8u : 0u);  // MarchLds::ctl: shared pool cursor
    uint32_t* s_tile = s_next + 1;                                     // work-list slot of the current tile
    uint32_t* s_veto = s_next + 2;
    float* s_off = reinterpret_cast<float*>(s_next + rml::kMarchCtlBytes / 4u);  // [16][2] screen offsets of the AA samples (wgsl:47-53)
    uint8_t* rmat = reinterpret_cast<uint8_t*>(s_next) + rml::kMarchCtlBytes + rml::kMarchOffBytes;  // MAT, tagged program: [V5_POOL] material per ray
    // MarchLds::pad: primitive mask of the current tile (a kernel without MAT never meets a tagged program: a fixed offset from s_next)
    uint32_t* s_mask = reinterpret_cast<uint32_t*>(rmat + (MAT && L.n_mrec != 0u ? V5_POOL : 0u));
    const bool tagged = MAT && L.n_mrec != 0u;                         // wave-uniform
    constexpr uint32_t TAP_IDLE = MAT ? 5u : 4u;                       // tap_t: 0..3 normal taps, 4 (MAT) material, else idle
    const CullTables cullt{t_cone, t_slab, s_veto, L.n_cone, L.n_slab};

    rm_uniforms u = L.u;
    if (L.frames) u = L.frames[blockIdx.z];  // wave-uniform
    const uint32_t tiles_x = (L.W + 7u) / 8u;
    const uint32_t* order = work.order + (size_t)blockIdx.z * n_tiles;
    uint32_t* counters = work.counters + 4u * blockIdx.z;
    const uint32_t n_active = counters[0];

    const V4 ro = matvec(u.inv_view, 0.0f, 0.0f, 0.0f, 1.0f);  // wgsl:39-40
    // (prune_scale_v5 and bound_scale_march_v5, written out: called here, even with their operands by value, they moved the
    // scalar spill counts of these kernels, some up)
    const float prune_scale = L.scene_scale + ((__builtin_fabsf(ro.x) + __builtin_fabsf(ro.y)) + __builtin_fabsf(ro.z));  // "Pruning"
    const float thr_c0 = step_thr_c0(prune_scale, ro.x, ro.y, ro.z);  // the wave-uniform part of a march step's threshold
    const float eps = 0.0001f;                                    // wgsl:136
    if (PROG_IN_LDS) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(L.prog);
        // program (generated code reads the records rotated by one dword: parameters first, lds_load4), then the unit table
        for (uint32_t k = tid; k < L.n_rec * 8u; k += 64u * WPT) lprog[SPEC ? ((k & ~7u) | ((k + 7u) & 7u)) : k] = src[k];
        stage_units(lprog + 8u * L.n_rec, L.prog + L.n_rec, L.n_grp, tid, 64u * WPT);  // (7 of a unit record's 8 dwords: it fits the same space)
        if constexpr (!SPEC) stage_tree(lprog + 8u * (L.n_rec + L.n_grp), L.prog + L.n_rec + L.n_grp, L.n_tree, tid, 64u * WPT);
    }
    // (the steps of stage_cull_tables, written out: the program's copy shares the first barrier, the tile loop's first barrier
    // closes the table build, and there are no aux rows)
    if (tid == 0u) *s_veto = 0u;
    if (tid < 16u) sample_offset(u, tid >> 2, tid & 3u, s_off[2u * tid], s_off[2u * tid + 1u]);  // two divisions per sample, once
    __syncthreads();
    if (L.flags & 1u)
        for (uint32_t k = tid; k < L.n_rec; k += 64u * WPT) cull_build_v5(L.prog[k], ro, L.min_dist, L.smooth_slack, t_cone, t_slab, s_veto, L.bounds);

    Prog prog;
    if constexpr (PROG_IN_LDS) prog.base = lprog;
    else prog.base = L.prog;

    // record i of the program as (opcode, parameters), wherever this kernel keeps it (SPEC: the rotated LDS copy)
    auto load_record = [&](uint32_t i, uint32_t& op, float (&p)[7]) {
        if constexpr (PROG_IN_LDS) {
            const uint32_t* r = lprog + 8u * i;
            op = r[SPEC ? 7u : 0u];
#pragma unroll
            for (int k = 0; k < 7; k++) p[k] = __uint_as_float(r[(SPEC ? 0u : 1u) + (uint32_t)k]);
        } else {
            prog.load(i, op, p);
        }
    };
    const float bound_scale = prune_scale + L.smooth_slack;  // scale of the coordinates the bounds are computed from
    const LdsF lprog_v = lds_vector_base(lprog);  // SPEC: the program's LDS copy, base address in a VGPR (see LdsF)
    uint32_t n_eval = 0u;  // diagnostics (pruned kernels compiled with statistics): leaves actually evaluated, per wave
    // Wave-level culling (above): the units of the program this wave has to evaluate at its live lanes' positions.  Generated
    // kernels know at compile time whether and how they cull; the interpreter kernels look at the launch (flags bit 3).
    const uint32_t* lunits = lprog + 8u * L.n_rec;  // the unit records behind the program (PROG_IN_LDS kernels only)
    auto units_needed = [&](float x, float y, float z, float thr, float extra_margin, bool is_live, unsigned long long live_mask) -> unsigned long long {
        if constexpr (SPEC) {
#if defined(RM_JIT_PRUNE_ON)
            return wave_cull_lattice(lunits, L.n_grp, x, y, z, thr, is_live, live_mask);
#elif defined(RM_JIT_BLEND_PRUNE)
            return wave_cull_blend(lunits, L.n_grp, L.unit_kmax, x, y, z, extra_margin, prune_scale, is_live, live_mask);
#else
            return ~0ull;
#endif
        } else if constexpr (LOOP == 2 || LOOP == 4) {  // (the masked loops are for lattice programs)
            return wave_cull_lattice(lunits, L.n_grp, x, y, z, thr, is_live, live_mask);
        } else if constexpr (LOOP == 1 || LOOP == 3) {
            return ~0ull;
        } else if constexpr (PROG_IN_LDS) {
            if ((L.flags & 8u) == 0u) return ~0ull;
            if (L.unit_mode == RM_UNITS_LATTICE) return wave_cull_lattice(lunits, L.n_grp, x, y, z, thr, is_live, live_mask);
            return wave_cull_blend(lunits, L.n_grp, L.unit_kmax, x, y, z, extra_margin, prune_scale, is_live, live_mask);
        } else {
            return ~0ull;
        }
    };
    // map_scene (wgsl:187-203) at one point per lane
    auto eval_scene = [&](float x, float y, float z, float thr, bool is_live, unsigned long long live_mask) -> float {
        float qx[1] = {x}, qy[1] = {y}, qz[1] = {z}, v[1];
        SqrtGuard tiny;
        if constexpr (SPEC) {  // straight-line code compiled for this program's structure (rm_jit.h)
            const unsigned long long need = units_needed(x, y, z, thr, 0.0f, is_live, live_mask);
            v[0] = RM_MAP_SCENE_STEP<true>(lprog_v, x, y, z, need, live_mask, tiny, n_eval);
            if (tiny.any_bad()) {
                // (an empty volatile asm keeps this a branch: for a program of one or two leaves the compiler otherwise
                // evaluates both forms at every step and selects -- a second square root and 16 more vector instructions)
                asm volatile("");
                uint32_t again = 0u;
                v[0] = RM_MAP_SCENE_STEP<false>(lprog_v, x, y, z, need, live_mask, tiny, again);
            }
        } else if (LOOP == 1 || LOOP == 2 || (LOOP == 0 && (L.flags & 4u))) {  // chain program (wave-uniform): the stack-free record loop
            const unsigned long long need = units_needed(x, y, z, thr, 0.0f, is_live, live_mask);
            const bool masked = LOOP == 0 ? (PROG_IN_LDS && (L.flags & 8u) != 0u) : LOOP == 2;  // (the unit records are staged in LDS with the program)
#ifdef RM_INTERP_STATS
            n_eval += (uint32_t)__builtin_popcountll(masked ? need : (L.n_rec >= 64u ? ~0ull : (1ull << L.n_rec) - 1ull));
#endif
            v[0] = map_scene_chain<true>(prog, L.n_rec, x, y, z, need, masked, tiny);
            if (tiny.any_bad()) v[0] = map_scene_chain<false>(prog, L.n_rec, x, y, z, need, masked, tiny);
        } else if (LOOP == 3 || LOOP == 4 || (LOOP == 0 && !EXT)) {  // tree program -- reference node types in any arrangement, all a kernel
                                                                      // without the extensions ever gets --: one dispatch per record
            const bool masked = LOOP == 0 ? (PROG_IN_LDS && (L.flags & 8u) != 0u) : LOOP == 4;
            if (masked) {  // ... over the records the wave's unit mask leaves (L.n_tree != 0)
                const unsigned long long need = units_needed(x, y, z, thr, 0.0f, is_live, live_mask);
                const TreeKeep k = tree_keep(lunits + 8u * L.n_grp, L.n_rec, need);
#ifdef RM_INTERP_STATS  // diagnostics build (tools/wave_stats.py --interp-stats): records executed, per wave
                n_eval += (uint32_t)(__builtin_popcountll(k.keep0) + __builtin_popcountll(k.keep1));
#endif
                v[0] = map_scene_tree_masked<true>(prog, spill, x, y, z, k.keep0, k.keep1, k.push0, k.push1, tiny);
                if (tiny.any_bad()) v[0] = map_scene_tree_masked<false>(prog, spill, x, y, z, k.keep0, k.keep1, k.push0, k.push1, tiny);
            } else {
                v[0] = map_scene_tree<true>(prog, L.n_rec, spill, x, y, z, tiny);
                if (tiny.any_bad()) v[0] = map_scene_tree<false>(prog, L.n_rec, spill, x, y, z, tiny);
            }
        } else if (PROG_IN_LDS && (L.flags & 8u)) {  // a blending chain: the general record machine over the units the wave's mask names
            const unsigned long long need = units_needed(x, y, z, thr, 0.0f, is_live, live_mask);
            const uint32_t* ranges = lunits + 7u * L.n_grp;  // row 7 of the unit table
            v[0] = map_scene_units<true, EXT>(prog, ranges, spill, x, y, z, need, tiny, L.value_spill_depth);
            if (tiny.any_bad())  // a sqrt argument outside the fast range (SqrtGuard): redo with the generic sqrt
                v[0] = map_scene_units<false, EXT>(prog, ranges, spill, x, y, z, need, tiny, L.value_spill_depth);
        } else {
            map_scene_multi<1, true, Prog, EXT>(prog, L.n_rec, spill, L.max_dist, qx, qy, qz, v, tiny, L.value_spill_depth);
            if (tiny.any_bad()) map_scene_multi<1, false, Prog, EXT>(prog, L.n_rec, spill, L.max_dist, qx, qy, qz, v, tiny, L.value_spill_depth);
        }
        return v[0];
    };

    // The first march step of EVERY ray of the frame evaluates the same point: pos = ro + rd * 0 (wgsl:88-94).
    // rm_tile_sort_v5 took it once per frame (f0); rays start from its outcome (wgsl:97-114 applied to f0):
    //   START_HIT    f0 < min_dist: the hit is at ro, the ray goes straight to its normal taps
    //   START_DONE   f0 > max_dist, or max_iter == 1: the loop ends without a hit
    //   START_MARCH  dist = 0 + f0, one iteration used
    // (only for finite rd: with a NaN / inf component rd * 0 is NaN and the ray starts the ordinary way)
    enum : uint32_t { START_MARCH = 0u, START_HIT = 1u, START_DONE = 2u };
    const float f0 = __uint_as_float(__builtin_amdgcn_readfirstlane(counters[2]));
    uint32_t start = START_DONE;
    if (L.max_iter != 0u)
        start = f0 < L.min_dist ? START_HIT : (f0 > L.max_dist || L.max_iter <= 1u) ? START_DONE : START_MARCH;
    const float inf_f = __uint_as_float(0x7F800000u);
    // The wave's anchor ("Pruning", anchored first step): a point of this launch and the reach of the value computed there; kept
    // by the kernels whose wave-level culling reads the threshold -- the generated lattice kernels, the interpreter's masked loops
#if defined(RM_JIT_PRUNE_ON)
    constexpr bool ANCHOR = SPEC;
#elif defined(RM_PRUNE_PLUMBING)
    constexpr bool ANCHOR = !SPEC && (LOOP == 2 || LOOP == 4);
#else
    constexpr bool ANCHOR = false;
#endif
    float anc_x = 0.0f, anc_y = 0.0f, anc_z = 0.0f, anc_t = inf_f;  // wave-uniform; never reset between tiles
    unsigned long long anc_due = 0ull;  // wave-uniform, all ones: rays were handed out, the next march evaluation is captured

    const unsigned long long t_start = L.stats ? __builtin_amdgcn_s_memrealtime() : 0ull;
    // (diagnostics, RM_OPT_WAVE_STATS; a generated kernel keeps them only when it was compiled for that: RM_NO_WAVE_STATS, rm_jit.h)
    uint32_t n_iter = 0u, n_live = 0u, n_prod = 0u, n_tiles_done = 0u;

  for (;;) {  // ---- next tile of the work list ----
    if (tid == 0u) {
        *s_tile = atomicAdd(&counters[1], 1u);
        *s_next = 0u;
        s_next[3] = 0u;  // "the per-ray miss tests clear nothing in this tile", see the production of rays below
    }
    __syncthreads();
    const uint32_t slot = *s_tile;
    if (slot >= n_active) break;
    const uint32_t tile = order[slot];
    const uint32_t tile_x = tile % tiles_x, tile_y = tile / tiles_x;
    n_tiles_done++;
    const unsigned long long tile_t0 = work.measured ? __builtin_amdgcn_s_memrealtime() : 0ull;

    // Ray r of the pool: pixel r & 63, AA sample r >> 6 (the resolve step reads res[] that way).  A produce round makes the 64
    // rays of one BATCH: the sixteen samples of a 2x2 block of pixels (lane: sample lane >> 2, pixel lane & 3 of the block) --
    // rays that stay within two pixels of each other march alike (they finish together: fewer idle lanes) and lie in a small
    // ball (wave-level culling tests the units against that ball).  Round 2's batch was one sample of all 64 pixels.
    if (lane < 16u) {
        const uint32_t k = lane & 7u, tx = tile_x * 8u + k, ty = tile_y * 8u + k;
        wxy[lane] = lane < 8u ? screen_x(tx < L.W ? tx : L.W - 1u, L.W)                                // edge tiles clamp
                              : screen_y(rm_global_row(L, ty < L.rows ? ty : L.rows - 1u), L.H);
    }
    // the tile's primitive mask, for the ray tests of the produce rounds: every wave stores the same word and reads it behind
    // its own fence (kept in LDS, not in a scalar register that would live through the march loop)
    if (lane == 0u) *s_mask = work.masks[(size_t)blockIdx.z * n_tiles + tile];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

    // lane state of a marching ray: evaluation point = ro + d * sc
    float dx = 0.f, dy = 0.f, dz = 0.f, sc = 0.f;
    // itr: the ray's id in the pool (bits 0-9) and the march steps it has taken (bits 10 and up; max_iter <= 65536) in ONE
    // register -- a step adds 1024, the loop bound compares with max_iter << 10 -- the one register between 6 and 5 waves per SIMD
    // ... and the lane's state in its top two bits: 0 marching, ITR_EMPTY idle (waiting for a ray), ITR_RETIRED nothing left to take
    constexpr uint32_t ITR_EMPTY = 0x80000000u, ITR_RETIRED = 0x40000000u;  // (a marching ray's itr stays below 2^27)
    uint32_t itr = ITR_EMPTY;
    auto lane_empty = [&]() { return (int32_t)itr < 0; };
    auto lane_marching = [&]() { return itr < ITR_RETIRED; };
    const uint32_t iter_limit = L.max_iter << 10;
    float thr_base = inf_f;  // SPEC: pruning threshold without its position term ("Pruning")
    // (a hit whose normal is being sampled keeps its state -- position, partial normal -- in LDS: tap phase, below)
    uint32_t rq_pos = 0u, rq_cnt = 0u, sq_n = 0u, hq_n = 0u;  // wave-uniform cursors: ready / miss / hit buffers
    uint32_t tap_t = TAP_IDLE, tap_n = 0u;                     // wave-uniform: tap phase step (TAP_IDLE = not in one), its entries
    bool pool_open = true;                                     // wave-uniform: the shared pool may still hold rays

    auto flush_misses = [&]() {  // floor / black for every waiting ray that ended without a hit (<= 64): wgsl:117-130
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (lane < sq_n) res[sq_rid[lane]] = miss_code(ro, sq_v[lane], sq_v[V5_SQ + lane], sq_v[2u * V5_SQ + lane]);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        sq_n = 0u;
    };

    for (;;) {
        if (tap_t == TAP_IDLE) {
            // ---- A. idle lanes take ready rays; when the buffer is empty it is refilled with the
            //         survivors of the next 64 candidates of the pool ----
            const unsigned long long want0 = __ballot(lane_empty());
            const unsigned long long live0 = __ballot(lane_marching());
            if (want0 != 0ull && (live0 == 0ull || (uint32_t)__popcll(want0) >= refill_min)) {
                unsigned long long want = want0;
                while (want != 0ull) {
                    if (rq_pos == rq_cnt) {  // buffer empty: produce
                        if (!pool_open) {
                            if (lane_empty()) itr = ITR_RETIRED;  // pool exhausted and buffer drained
                            break;
                        }
                        uint32_t base = 0u;
                        if (lane == 0u) base = atomicAdd(s_next, 64u);
                        base = __builtin_amdgcn_readfirstlane(base);
                        if (base >= V5_POOL) { pool_open = false; continue; }
                        n_prod++;
                        // batch -> block of the 4x4 blocks of the tile: the corners first, then the centre (see test_rays below)
                        const uint32_t blk = (uint32_t)(0xEDB87421A965FC30ull >> (4u * (base >> 6))) & 15u;
                        // (the lane's part of these is recomputed per round: hoisted out of the loop it would sit in registers through
                        // the four-tap function, whose pressure decides between 6 and 5 waves per SIMD)
                        uint32_t ln = lane;
                        asm volatile("" : "+v"(ln));
                        const uint32_t bpx = 2u * (blk & 3u) + (ln & 1u), bpy = 2u * (blk >> 2) + ((ln >> 1) & 1u), s = ln >> 2;
                        const uint32_t r = s * 64u + bpy * 8u + bpx;
                        float gx, gy, gz;
                        gen_ray_at<true>(u.inv_proj, u.inv_view, ro, wxy[bpx], wxy[8u + bpy], s_off[2u * s], s_off[2u * s + 1u], gx, gy, gz);
                        const bool finite_d = __builtin_fabsf(gx) < inf_f && __builtin_fabsf(gy) < inf_f && __builtin_fabsf(gz) < inf_f;
                        // The miss tests are optional (a ray they do not clear is marched and ends as the same miss): in a tile
                        // the scene covers completely they clear nothing -- 92 % of the rays that reach this kernel are marched --
                        // so once the batches of the tile's four CORNER blocks (the first four of the pool) went through without
                        // a single ray cleared, the rest of the tile's batches skip them.
                        const bool test_rays = (L.flags & 1u) != 0u && __builtin_amdgcn_readfirstlane(s_next[3]) < 4u;
                        bool culled = L.max_iter == 0u || (start == START_DONE && finite_d) || (test_rays && ray_misses_scene_v5(cullt, __builtin_amdgcn_readfirstlane(*s_mask), gx, gy, gz));
#if !defined(RM_JIT_TU) || defined(RM_JIT_BOUND_WALK)  // a generated kernel carries it only if its program's structure can use it
                        if (test_rays && (L.flags & 32u) && (*s_veto & 1u) == 0u && bound_scale < 1.0e12f && __ballot(!culled) != 0ull)  // "Miss test on lower bounds"
                            culled = culled || ray_misses_by_bounds_v5<false>(load_record, L.n_rec, ro, gx, gy, gz, L.min_dist, bound_scale);
#endif
                        if (test_rays && base < 256u && __ballot(culled) == 0ull && lane == 0u) atomicAdd(&s_next[3], 1u);
                        if (culled) res[r] = miss_code(ro, gx, gy, gz);  // never marched: wgsl:117-130 only
                        const unsigned long long keep = __ballot(!culled);
                        if (!culled) {
                            const uint32_t e = lane_rank(keep);
                            rq_rid[e] = r;
                            rq_d[e] = gx; rq_d[V5_RQ + e] = gy; rq_d[2u * V5_RQ + e] = gz;
                        }
                        rq_pos = 0u;
                        rq_cnt = (uint32_t)__popcll(keep);
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                        continue;
                    }
                    const uint32_t avail = rq_cnt - rq_pos, n_want = (uint32_t)__popcll(want);
                    if (lane_empty()) {
                        const uint32_t rank = lane_rank(want);
                        if (rank < avail) {
                            const uint32_t e = rq_pos + rank;
                            const uint32_t rid = rq_rid[e];
                            dx = rq_d[e]; dy = rq_d[V5_RQ + e]; dz = rq_d[2u * V5_RQ + e];
                            const bool finite_d = __builtin_fabsf(dx) < inf_f && __builtin_fabsf(dy) < inf_f && __builtin_fabsf(dz) < inf_f;
                            // The shared first step applies to finite rd that neither hit nor ended there (START_MARCH);
                            // everything else takes its own first step: rd * 0 = NaN, or the hit at ro (rare: the camera
                            // inside a solid), which then goes through the ordinary hit path.
                            const bool shared = finite_d && start == START_MARCH;
                            sc = shared ? 0.0f + f0 : 0.0f;  // dist (wgsl:88), dist += scene_dist (wgsl:114)
                            itr = rid | (shared ? 1024u : 0u);
                            thr_base = shared ? __builtin_fabsf(f0) * 2.00002f : inf_f;
                            if constexpr (ANCHOR) {  // the step's own expression for its first point: the same bits
                                if (shared) thr_base = anchor_thr_base(thr_base, ro.x + dx * sc, ro.y + dy * sc, ro.z + dz * sc, anc_x, anc_y, anc_z, anc_t);
                                thr_base = handout_thr_base(thr_base, thr_c0);  // (after the minimum: both of its sides carry c0)
                            }
                        }
                    }
                    rq_pos += n_want < avail ? n_want : avail;
                    if constexpr (ANCHOR) anc_due = ~0ull;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    want = __ballot(lane_empty());
                }
            }
            // ---- hits waiting for their normal: a tap phase runs when 64 are waiting, or when nothing else is left ----
            const bool any_live = __ballot(lane_marching()) != 0ull;
            if (!any_live && __ballot(lane_empty()) != 0ull) continue;  // idle lanes remain: force a refill round
            if (hq_n >= 64u || (!any_live && hq_n != 0u)) {
                tap_n = hq_n < 64u ? hq_n : 64u;
                hq_n -= tap_n;  // the most recent tap_n entries: [hq_n, hq_n + tap_n); nothing is pushed during the phase
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                tap_t = 0u;
            } else if (!any_live) {
                break;  // every lane retired, nothing waiting
            }
        }
        const bool tapping = tap_t != TAP_IDLE;  // wave-uniform
        if constexpr (MAT) {
            if (tap_t == 4u) {  // the normals of this batch are complete (tn): which material does each hit carry?
                const uint32_t e = hq_n + lane;
                const float hx = hq_v[e], hy = hq_v[V5_HQ + e], hz = hq_v[2u * V5_HQ + e];
#ifdef RM_JIT_MATERIAL_WALK
                SqrtGuard mtiny;
                uint32_t m = map_scene_material_spec<true>(L.mprog, hx, hy, hz, mtiny);
                if (mtiny.any_bad()) m = map_scene_material_spec<false>(L.mprog, hx, hy, hz, mtiny);
#else
                const uint32_t m = map_scene_material(L.mprog, L.n_mrec, spill, L.mat_value_depth, hx, hy, hz);
#endif
                if (lane < tap_n) {
                    const uint32_t r = hq_rid[e] & 1023u;
                    res[r] = shade_hit<true>(tn[lane], tn[64u + lane], tn[128u + lane], hx, hy, hz);  // wgsl:98-103
                    rmat[r] = (uint8_t)m;
                }
                tap_t = TAP_IDLE;
                continue;
            }
        }

#ifdef RM_JIT_TAPS4
        if (tapping) {  // all four normal taps of the batch in one pass over the program (wgsl:135-144)
            const uint32_t e = hq_n + lane;
            const float cx = hq_v[e], cy = hq_v[V5_HQ + e], cz = hq_v[2u * V5_HQ + e];
            const bool live4 = lane < tap_n;
            // |F(tap)| <= |sd_hit| + eps sqrt(3) + error: the threshold of a tap ("Pruning"); the far test runs at c,
            // another eps sqrt(3) and one more leaf-evaluation error away from every tap
            const float m = kPruneAbs * (prune_scale + (((__builtin_fabsf(cx) + __builtin_fabsf(cy)) + __builtin_fabsf(cz)) + 1.0e-3f));
            const float thr_c = __uint_as_float(hq_rid[e] & ~1023u) * 1.00001f + 3.5e-4f + (m + m);
            float f[4];
            SqrtGuard tiny;
            const unsigned long long live4_m = __builtin_amdgcn_ballot_w64(live4);
            // the units are decided at the hit positions c, eps sqrt(3) from every tap: the threshold (lattice programs) or
            // the margin (programs that blend) carries that distance twice over
            const unsigned long long need4 = units_needed(cx, cy, cz, thr_c, 3.5e-4f, live4, live4_m);
            map_scene_taps<true>(lprog_v, cx, cy, cz, need4, live4_m, tiny, f);
            if (tiny.any_bad()) map_scene_taps<false>(lprog_v, cx, cy, cz, need4, live4_m, tiny, f);
#ifndef RM_NO_WAVE_STATS
            n_iter++;
            n_live += (uint32_t)__popcll(live4_m);
#endif
            // n = ((k0 f0 + k1 f1) + k2 f2) + k3 f3, k = (+,-,-), (-,-,+), (-,+,-), (+,+,+); products with +-1 are exact
            const float nx = ((f[0] + -f[1]) + -f[2]) + f[3];
            const float ny = ((-f[0] + -f[1]) + f[2]) + f[3];
            const float nz = ((-f[0] + f[1]) + -f[2]) + f[3];
            if (tagged) {
                tn[lane] = nx; tn[64u + lane] = ny; tn[128u + lane] = nz;
                tap_t = 4u;  // the material phase follows
            } else {
                // (the hit position is read again rather than kept in three registers through the four-tap function, whose
                // pressure is the kernel's peak: the acquire keeps the compiler from forwarding the earlier loads)
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if (live4) res[hq_rid[e] & 1023u] = shade_hit<true>(nx, ny, nz, hq_v[e], hq_v[V5_HQ + e], hq_v[2u * V5_HQ + e]);  // wgsl:98-103
                tap_t = TAP_IDLE;
            }
            continue;
        }
#endif
        // ---- B. map_scene evaluations: march steps of the live rays, or the normal taps of the waiting hits ----
        // An inner loop of its own: evaluation follows evaluation until something else is due -- a refill, a tap phase, the end
        // of the tile's rays --, and that can only change when a ray finishes.  Section A's questions (who is idle, who is live,
        // how many hits wait) are then asked once per finished ray instead of once per step: a dozen scalar instructions and a
        // handful of branches less per march step, in a kernel whose scalar side is as busy as its vector side (a CU has one
        // scalar unit for four SIMDs: 4.3 cycles per scalar instruction per SIMD, profiles/r03_ubench_scalar_issue_cycles.txt).
        // The sequence of evaluations is the one the flat loop produced.
        uint32_t n_idle = tapping ? 0u : (uint32_t)__popcll(__ballot(lane_empty()));  // wave-uniform: lanes waiting for a ray
        for (;;) {
            // (the interpreter kernels keep ONE copy of the evaluation for march steps and taps: their record loops are large, and the
            // loop unswitched on `tapping` costs the lean kernel its registers)
            bool tapping_i = tapping;
            if constexpr (!SPEC) {
                uint32_t t = tapping ? 1u : 0u;
                asm volatile("" : "+v"(t));
                tapping_i = __builtin_amdgcn_readfirstlane(t) != 0u;
            }
            float ex, ey, ez, thr = inf_f;
            bool is_live;
            uint32_t sgx = 0u, sgy = 0u, sgz = 0u;
            const uint32_t he = hq_n + lane;  // this lane's hit-buffer entry in a tap phase (< V5_HQ for every lane)
            if (tapping_i) {  // pos + k_t * eps (wgsl:138-141); k_t * eps = +-eps exactly
                tap_signs(tap_t, sgx, sgy, sgz);
                ex = hq_v[he] + __uint_as_float(__float_as_uint(eps) ^ sgx);
                ey = hq_v[V5_HQ + he] + __uint_as_float(__float_as_uint(eps) ^ sgy);
                ez = hq_v[2u * V5_HQ + he] + __uint_as_float(__float_as_uint(eps) ^ sgz);
                is_live = lane < tap_n;
#ifdef RM_PRUNE_PLUMBING
                // the tap is eps * sqrt(3) away from the hit position, where the scene value was sd_hit ("Pruning")
                thr = __uint_as_float(hq_rid[he] & ~1023u) * 1.00001f + 1.75e-4f +
                      kPruneAbs * (prune_scale + ((__builtin_fabsf(ex) + __builtin_fabsf(ey)) + __builtin_fabsf(ez)));
#endif
            } else {
                ex = ro.x + dx * sc; ey = ro.y + dy * sc; ez = ro.z + dz * sc;  // wgsl:91
                is_live = lane_marching();
                if constexpr (ANCHOR) thr = step_thr(thr_base, sc);  // ("Pruning", the position term along a ray)
                else thr = thr_base + kPruneAbs * (prune_scale + ((__builtin_fabsf(ex) + __builtin_fabsf(ey)) + __builtin_fabsf(ez)));
            }
            const unsigned long long live_m = __builtin_amdgcn_ballot_w64(is_live);
#ifndef RM_NO_WAVE_STATS
            n_iter++;
            n_live += (uint32_t)__popcll(live_m);
#endif
            const float sd = eval_scene(ex, ey, ez, thr, is_live, live_m);

            if (tapping_i) {  // n (+)= k_t * f; products with +-1 are exact (wgsl:138-143)
                const float vx = __uint_as_float(__float_as_uint(sd) ^ sgx);
                const float vy = __uint_as_float(__float_as_uint(sd) ^ sgy);
                const float vz = __uint_as_float(__float_as_uint(sd) ^ sgz);
                // the partial sum waits in LDS between taps, not in three registers that every march iteration would carry
                const float nx = tap_t == 0u ? vx : tn[lane] + vx;
                const float ny = tap_t == 0u ? vy : tn[64u + lane] + vy;
                const float nz = tap_t == 0u ? vz : tn[128u + lane] + vz;
                if (++tap_t == 4u && !tagged) {
                    if (is_live) res[hq_rid[he] & 1023u] = shade_hit<true>(nx, ny, nz, hq_v[he], hq_v[V5_HQ + he], hq_v[2u * V5_HQ + he]);  // wgsl:98-103
                    tap_t = TAP_IDLE;
                    break;
                }
                tn[lane] = nx; tn[64u + lane] = ny; tn[128u + lane] = nz;
                if (tap_t == 4u) break;  // (tagged program: the material phase follows)
                continue;                // the next tap of the same hits
            }

            // ---- C. march bookkeeping (wgsl:97-114); finished rays leave their lane ----
            // Written on wave masks (64-bit scalars) with explicit selects: left to itself the compiler turned the lane
            // predicates into 0/1 integers and back (17 vector instructions for what takes 7).
            const unsigned long long hit_mask = live_m & __ballot(sd < L.min_dist);                       // wgsl:97
            const unsigned long long on_m = live_m & ~hit_mask;                                           // (a NaN is not a hit)
            const unsigned long long esc_m = on_m & __ballot(sd > L.max_dist);                            // wgsl:109-111
            const unsigned long long go_m = on_m & ~esc_m;
            sc = select_by_mask(sc, sc + sd, go_m);                                                       // wgsl:114
            itr = select_by_mask(itr, itr + 1024u, go_m);
#ifdef RM_PRUNE_PLUMBING  // only pruning kernels read it
            thr_base = select_by_mask(thr_base, ANCHOR ? step_thr_base(sd, thr_c0) : __builtin_fabsf(sd) * 2.00002f, go_m);  // the next point is |sd| |rd| away
#endif
            const unsigned long long miss_mask = esc_m | (go_m & __ballot(itr >= iter_limit));             // loop bound, wgsl:90
            const unsigned long long done_m = hit_mask | miss_mask;
            if constexpr (ANCHOR) {
                if ((done_m | anc_due) == 0ull) continue;  // (as below; one scalar OR is all a step pays for the capture)
                if (anc_due != 0ull) {  // first evaluation after rays were handed out: the first live lane's point and value
                    const int al = (int)__builtin_ctzll(live_m);  // (section A leaves a marching lane: live_m != 0)
                    const float at = anchor_reach(ex, ey, ez, sd, prune_scale);
                    anc_x = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(ex), al));
                    anc_y = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(ey), al));
                    anc_z = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(ez), al));
                    anc_t = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(at), al));
                    anc_due = 0ull;
                    if (done_m == 0ull) continue;
                }
            }
            if (done_m == 0ull) continue;  // every live ray goes on: nothing section A asks about has changed
            const bool hit = is_live && sd < L.min_dist, miss = lane_of(miss_mask, lane);
            if (hit_mask != 0ull) {  // -> hit buffer (capacity 128: a tap phase takes 64 as soon as 64 are waiting)
                if (hit) {
                    const uint32_t e = hq_n + lane_rank(hit_mask);
#ifdef RM_PRUNE_PLUMBING
                    // |sd| of the hit, rounded up to 22 bits, rides in the upper bits of the entry's ray id (< 1024): the
                    // pruning threshold of its normal taps ("Pruning"); a NaN stays a NaN (nothing is skipped then)
                    hq_rid[e] = (itr & 1023u) | ((__float_as_uint(__builtin_fabsf(sd)) + 1023u) & ~1023u);
#else
                    hq_rid[e] = itr & 1023u;
#endif
                    hq_v[e] = ex; hq_v[V5_HQ + e] = ey; hq_v[2u * V5_HQ + e] = ez;
                    itr = ITR_EMPTY;
                }
                hq_n += (uint32_t)__popcll(hit_mask);
            }
            if (miss_mask != 0ull) {
                const uint32_t n_miss = (uint32_t)__popcll(miss_mask);
                if (sq_n + n_miss > V5_SQ) flush_misses();
                if (miss) {
                    const uint32_t e = sq_n + lane_rank(miss_mask);
                    sq_rid[e] = itr & 1023u;
                    sq_v[e] = dx; sq_v[V5_SQ + e] = dy; sq_v[2u * V5_SQ + e] = dz;
                    itr = ITR_EMPTY;
                }
                sq_n += n_miss;
            }
            // back to section A when it has something to do: no ray left marching, enough idle lanes for a refill (refill_min; when
            // the pool is exhausted A retires them), or 64 hits waiting for their normals
            n_idle += (uint32_t)__popcll(done_m);
            if ((live_m & ~done_m) == 0ull || n_idle >= refill_min || hq_n >= 64u) break;
        }
    }
    if (sq_n != 0u) flush_misses();
    __syncthreads();  // all waves of the tile are done: res[] is complete

    // ---- resolve: one pixel per thread, samples in the reference order (wgsl:44-45, 68-69) ----
    for (uint32_t p = tid; p < 64u; p += 64u * WPT) {
        const uint32_t px = tile_x * 8u + (p & 7u), py = tile_y * 8u + (p >> 3);
        if (px < L.W && py < L.rows) {
            // the 48 gamma square roots of a pixel (wgsl:68) take the short form of the leaves' sqrt (rm_interp.h sqrt_rn_fast:
            // the same bits for every argument its guard lets through); a colour it does not -- negative or NaN from a material
            // table, infinite from a table or from a degenerate normal (below) -- sends the pixel through the generic form.
            // Without a table (kernels compiled with the range proofs have none; rm_interp.h "Range proofs") a colour is 0.4 / 0.7 /
            // 0.1 times a code that is max(0.02, dot) -- a NaN dot is dropped by the maximum --, or 0.1 / 0.2 plus 0 or 0.2 for the
            // floor, or 0: never negative, never NaN, and zero or at least 2e-3, so the LOWER side is not guarded.  The UPPER side
            // is, on one channel: shade_hit divides by a zero root when the three squares of a normal underflow (tap values that
            // differ by less than 2^-75: radii that small around a camera inside the solid reach it), the dot may then be +inf, and
            // the three colours are infinite together (0.7 code does not overflow for a finite code): the green one speaks for all.
            constexpr bool kGammaLo = MAT || !kRangeProved, kGammaHiAll = kGammaLo;
            auto sum_samples = [&](auto fast_tag, float& tr, float& tg, float& tb, SqrtGuard& guard) {
                constexpr bool FAST = decltype(fast_tag)::value;
                tr = 0.0f; tg = 0.0f; tb = 0.0f;
#pragma unroll 4
                for (uint32_t s = 0; s < 16u; s++) {
                    const float code = res[s * 64u + p];
                    float cr, cg, cb;
                    if (code >= 0.0f) {  // hit: (0.4,0.7,0.1) * k  (wgsl:105)
                        cr = 0.4f * code; cg = 0.7f * code; cb = 0.1f * code;
                        if constexpr (MAT) {
                            if (tagged) {  // extension: the albedo of the material the surface carries
                                const float4 al = L.materials[rmat[s * 64u + p]];
                                cr = al.x * code; cg = al.y * code; cb = al.z * code;
                            }
                        }
                    } else if (code > -2.5f) {  // floor (wgsl:127)
                        const float g = 0.2f * (-1.0f - code);
                        cr = 0.1f + g; cg = 0.1f + g; cb = 0.2f + g;
                    } else {
                        cr = 0.0f; cg = 0.0f; cb = 0.0f;  // wgsl:130
                    }
                    tr += sqrt_sel<FAST, true, kGammaLo, kGammaHiAll>(cr, guard);
                    tg += sqrt_sel<FAST, true, kGammaLo, true>(cg, guard);
                    tb += sqrt_sel<FAST, true, kGammaLo, kGammaHiAll>(cb, guard);
                }
            };
            float tr, tg, tb;
            SqrtGuard gamma_guard;
            sum_samples(TrueTag(), tr, tg, tb, gamma_guard);
            if (gamma_guard.bad()) sum_samples(FalseTag(), tr, tg, tb, gamma_guard);  // per lane: the rare pixel, not the wave
            store_pixel(L, blockIdx.z, (size_t)py * L.W + px, tr / 16.0f, tg / 16.0f, tb / 16.0f);  // wgsl:73-75
        }
    }
    if (work.measured && tid == 0u) {
        const unsigned long long dt = __builtin_amdgcn_s_memrealtime() - tile_t0;
        work.measured[(size_t)blockIdx.z * n_tiles + tile] = dt > 0xFFFFFFFFull ? 0xFFFFFFFFu : (dt == 0ull ? 1u : (uint32_t)dt);
    }
    __syncthreads();  // res[] / rings / cursor are reused by the next tile
  }
    if (L.stats && lane == 0u) {
        unsigned long long* st = L.stats + 4ull * (((size_t)blockIdx.z * gridDim.x + blockIdx.x) * WPT + wave);
        st[0] = t_start;
        st[1] = __builtin_amdgcn_s_memrealtime();
        st[2] = ((unsigned long long)n_tiles_done << 32) | n_iter;
#ifdef RM_JIT_WALK_COUNTER  // RM_JIT_PRUNE_STATS=5: evaluations that took the single-unit path -- a count that may well be zero
        st[3] = ((unsigned long long)n_eval << 32) | n_live;
#else
        st[3] = ((unsigned long long)(n_eval != 0u ? n_eval : n_prod) << 32) | n_live;
#endif
    }
}

template <class Prog, bool PROG_IN_LDS, int WPT, bool EXT>
__global__ __launch_bounds__(64 * WPT) void rm_render_v5(RmLaunch L, V5Work work, uint32_t n_tiles, uint32_t refill_min) {
    rm_render_v5_body<Prog, PROG_IN_LDS, WPT, EXT, false, EXT>(L, work, n_tiles, refill_min);
}
// The interpreter for reference-only programs staged in LDS -- north_star's design, and what runs while a structure compiles --
// with its vector registers capped at 80 (6 waves per SIMD, which is also what its LDS footprint allows): left alone the
// allocator takes 81 and a sixth of the occupancy (march kernel of the metric frame 0.83 -> 0.87 ms).
template <int WPT, int LOOP>
__global__ __launch_bounds__(64 * WPT) __attribute__((amdgpu_waves_per_eu(6, 8)))
void rm_render_v5_lean(RmLaunch L, V5Work work, uint32_t n_tiles, uint32_t refill_min) {
    rm_render_v5_body<ProgLds, true, WPT, false, false, false, LOOP>(L, work, n_tiles, refill_min);
}

// ---------------------------------------------------------------------------------------------
// Pre-pass: a workgroup of four waves owns a block of V5_PRE_BLOCK consecutive tiles.  It builds the
// tables once, settles what it can per TILE (lane = tile), and its waves then claim the block's tiles
// from a counter: a settled tile is filled with its constant, every other tile gets the per-pixel
// test (one wave per tile, lane = pixel).
//
// Per pixel, each lane decides whether ALL 16 AA rays of its pixel provably miss the scene, with one test per
// primitive instead of sixteen.  The 16 sample points are an affine 4x4 grid on the screen and
// pt_world.xyz - ro.xyz is affine in the screen position (two mat-vecs, wgsl:56-61), so the 16 ray
// directions lie in the convex cone spanned by the four extreme samples (i, j in {0, 3}).  With the
// unit directions e_0..e_3 of those four, c = normalize(e_0 + .. + e_3) and rho = max |e_i - c|,
// every sample direction e of the pixel satisfies |e - c| <= rho (the distance to a fixed point is
// maximal at a vertex of a convex spherical polygon smaller than a hemisphere; rho < 0.05 is required,
// which also rejects a pixel whose parallelogram contains the origin).  Then for a primitive with
// bounding cone (m, s) -- a ray clears it iff m.e < s, see cull_build_v5 --
//     m.e = m.c + m.(e - c) <= m.c + |m| rho,
// so  m.c + |m| rho < s  clears the primitive for the whole pixel.  Boxes get a second chance when
// that fails: a point P of any of the pixel's rays inside the (margin-inflated) box has |P| <= D =
// |m| + radius, and the centre ray passes within D rho of it, so if the centre ray misses the box
// inflated by a further D rho, every ray of the pixel misses the box.  rho carries 0.1 % + 2e-6 of
// slack for the rounding of e_i and c, and the frame's cone_noise_v5 for that of the mat-vecs (below).
//
// Per tile, the same three proofs (clear of the tables, sky, one checker cell) run on the rectangle of
// the tile's 32 x 32 sample positions; none of them needs the rectangle to be one pixel's grid.  What
// has to be re-examined is that a tile's samples are NOT one affine grid: every pixel centre
// screen_x(px), screen_y(py) and every sum centre + offset is rounded on its own.  The proofs never
// use the grid, though, only that every sample position lies in the rectangle spanned by the four
// extreme ones, and that holds exactly, with no slack: a correctly rounded operation is monotone in
// each operand, so screen_x is non-decreasing in px, screen_y non-increasing in py, and
// fl(centre + offset) is monotone in both; the sample offsets are monotone in (i, j).  Hence every
// x the march computes in the tile lies in [fl(screen_x(8 tx) + min offset), fl(screen_x(8 tx + 7) +
// max offset)], both ends being values the march computes itself (for an edge tile the far end belongs
// to a pixel outside the frame: a superset), and likewise for y, provided the tile's eight rows are
// consecutive rows of the frame (strips of a height that is no multiple of 8 break that: no tile
// verdicts then).  The remaining error is that of the two mat-vecs and the normalisation between a
// position and its direction.  It is absolute -- some 1e-7 of `mag`, whatever the rectangle's size --
// and it is what the 2e-6 in rho, the 1e-5 mag of the sky rule and the E = 4e-6 mag of the cell rule
// were sized for: they cover an interior sample and a corner of a tile as they cover those of a pixel,
// and the relative 0.1 % of rho only grows with the rectangle.  So the constants stand as they are,
// and the bounds bx, by of |x|, |y| that `mag` is built from are taken over the tile's rectangle.
// At rho >= 0.05 (frames of a few dozen pixels) a tile has no usable cone and nothing is settled per tile.
// The 2e-6 of rho covers the normalisations, NOT the mat-vecs: their error is absolute in the un-normalised direction, up to
// 1e-6 of `mag` per component (13 roundings of 2^-24 on the way from a position to pt_world - ro, each of a partial sum that
// `mag` bounds), and for the reference camera near the origin that is a few 1e-6 -- but `mag` grows with the camera's distance
// from the origin and with entries of the matrices that cancel (1e5 and -1e5 in one row of inv_proj quantise pt_view to 2^-7,
// several sample pitches: the samples between the corners then leave the corners' cone by 3e-3).  cone_noise_v5 bounds that error
// once per frame and rect_cone_v5 adds it to rho, twice (the corners' own and the sample's) over the shortest corner: a block
// whose noise is not small against a rectangle's directions gets no cone.
//
// A tile is settled per tile iff the tables clear its cone (the lower-bound walk of a blending program
// stays per pixel) and its samples are all sky or all in one cell.  It gets the constant the per-pixel
// path would have written -- zeros, or the sum of sixteen equal gamma values over 16 -- and cost 0.
//
// cost = number of pixels that are not provably clear (0..64).  A tile with cost 0 is finished
// here: its wave sums the 16 gamma-corrected floor colours of every pixel in the reference's order
// (wgsl:44-45, 68-69, 73-75) and writes it.  Tiles with cost > 0 go on the work list; the march
// kernel repeats the (sharper) test per ray.  76 % of the tiles of the metric frame end here, 60.5 % of
// all tiles settled per tile (tools/prepass_tile_classes.py; tests/test_gpu_prepass_tiles.py).
// ---------------------------------------------------------------------------------------------
constexpr uint32_t V5_PRE_TILES = 4u;  // waves per pre-pass workgroup, one tile at a time each
// Tiles per workgroup.  The waves claim them one by one (expensive tiles are neighbours: handing each wave a fixed four made the
// kernel slower, 60 -> 75 us).  The block size also fixes how full the one classifying wave is (lane = tile: 32 of its 64 lanes,
// while the other three waves wait at the barrier) and how often the prologue is paid.  16 and 64 both measured slower than 32 on
// the headline (profiles/r11_prepass_tile_classes_ab.txt); why was not profiled.
constexpr uint32_t V5_PRE_BLOCK = 32u;
static_assert(V5_PRE_BLOCK >= 1u && V5_PRE_BLOCK <= 64u, "one wave classifies the block, lane = tile");

#if !defined(RM_JIT_TU)  // not part of a specialised translation unit (rm_jit.h)
// The cone of a rectangle of sample positions.  px[a] + ox[a], py[b] + oy[b] (a, b in {0, 1}; added as gen_ray adds a pixel centre
// and a sample offset) are its extreme positions; corner c is (a, b) = (c & 1, c >> 1).  cone_out: (unit centre direction, rho) of
// the directions through the rectangle; rho = NaN when the cone is not usable.  corner[c]: pt_world.xyz - ro.xyz of corner c,
// as gen_ray computes it before its normalisation; the caller's sky / floor tests reuse them.  m_proj / m_view: the matrices (in
// vector registers).  noise: cone_noise_v5 of the frame.  Returns whether the cone is usable.
RM_DEV bool rect_cone_v5(const float* m_proj, const float* m_view, const V4& ro, const float (&px)[2], const float (&py)[2], const float (&ox)[2],
                         const float (&oy)[2], float noise, float (&cone_out)[4], float (&corner)[4][3]) {
    float cx = 0.0f, cy = 0.0f, cz = 0.0f, ex[4], ey[4], ez[4], inv_hi = 0.0f;
#pragma unroll
    for (uint32_t c = 0; c < 4u; c++) {
        gen_ray_unnormalized_at(m_proj, m_view, ro, px[c & 1u], py[c >> 1], ox[c & 1u], oy[c >> 1], ex[c], ey[c], ez[c]);
        corner[c][0] = ex[c]; corner[c][1] = ey[c]; corner[c][2] = ez[c];
        const float inv = __builtin_amdgcn_rsqf(__builtin_fmaf(ez[c], ez[c], __builtin_fmaf(ey[c], ey[c], ex[c] * ex[c])));  // (as unit_dir)
        ex[c] *= inv; ey[c] *= inv; ez[c] *= inv;
        inv_hi = fmax_(inv_hi, inv);  // 1 / the shortest corner; every sample is at least 0.998 of that long (rho < 0.05)
        cx += ex[c]; cy += ey[c]; cz += ez[c];
    }
    unit_dir(cx, cy, cz);
    float rho2 = 0.0f;
#pragma unroll
    for (uint32_t c = 0; c < 4u; c++) {
        const float ax = ex[c] - cx, ay = ey[c] - cy, az = ez[c] - cz;
        rho2 = fmax_(rho2, __builtin_fmaf(az, az, __builtin_fmaf(ay, ay, ax * ax)));
    }
    const float rho = __builtin_fmaf(2.2f * noise, inv_hi, __builtin_sqrtf(rho2) * 1.001f + 2.0e-6f);
    // NaN anywhere above (zero / non-finite directions) makes this false; v_max drops a NaN operand, so
    // the corners are checked one by one as well
    bool cone_ok = rho < 0.05f;
#pragma unroll
    for (uint32_t c = 0; c < 4u; c++) cone_ok = cone_ok && (ex[c] - cx) * (ex[c] - cx) < 1.0f && (ey[c] - cy) * (ey[c] - cy) < 1.0f && (ez[c] - cz) * (ez[c] - cz) < 1.0f;
    cone_out[0] = cx; cone_out[1] = cy; cone_out[2] = cz;
    cone_out[3] = cone_ok ? rho : __uint_as_float(0x7FC00000u);
    return cone_ok;
}
// How far rounding can move a sample's pt_world.xyz - ro.xyz from the affine image of its screen position (Euclidean; the same
// for every sample of a W x H frame): 1e-6 of the sum over the three components of |ro| + |inv_view row| . (|inv_proj| (|x|, |y|, 1,
// 1)), with |x|, |y| bounded for every position a tile's rectangle can have (its far corner may lie 7 pixels outside the frame).
RM_DEV float cone_noise_v5(const rm_uniforms& u, const V4& ro, uint32_t W, uint32_t H) {
    const float bx = (1.0f + 16.0f / (float)W) + 0.75f / __builtin_fabsf(u.viewport_extent[0]);
    const float by = (1.0f + 16.0f / (float)H) + 0.75f / __builtin_fabsf(u.viewport_extent[1]);
    float mag = (__builtin_fabsf(ro.x) + __builtin_fabsf(ro.y)) + __builtin_fabsf(ro.z);
#pragma unroll
    for (int k = 0; k < 4; k++)
        mag += ((__builtin_fabsf(u.inv_view[4 * k]) + __builtin_fabsf(u.inv_view[1 + 4 * k])) + __builtin_fabsf(u.inv_view[2 + 4 * k])) *
               (((__builtin_fabsf(u.inv_proj[k]) * bx + __builtin_fabsf(u.inv_proj[k + 4]) * by) + __builtin_fabsf(u.inv_proj[k + 8])) +
                __builtin_fabsf(u.inv_proj[k + 12]));
    return 1.0e-6f * mag;  // (anything non-finite ends up in rho and fails the cone)
}
// One entry of the cone test, cone (c, rho) of rect_cone_v5.  Cone entry k: every direction of the cone clears it iff
// m.c + |m| rho < s (NaN -> not clear).
RM_DEV bool cone_clears_cone_entry_v5(const CullTables& T, const float2* aux, uint32_t k, float cx, float cy, float cz, float rho) {
    const float4 a = T.cone[k];  // wave-uniform address: LDS broadcast
    const float t = __builtin_fmaf(aux[k].x, rho, __builtin_fmaf(a.z, cz, __builtin_fmaf(a.y, cy, a.x * cx)));
    return t < a.w;
}
// Slab entry k, its bounding sphere: as a cone entry.
RM_DEV bool cone_clears_slab_sphere_v5(const CullTables& T, const float2* aux, uint32_t k, float cx, float cy, float cz, float rho) {
    const float4 c = T.slab[3u * k + 2u];
    const float t = __builtin_fmaf(aux[T.n_cone + k].x, rho, __builtin_fmaf(c.z, cz, __builtin_fmaf(c.y, cy, c.x * cx)));
    return t < c.w;
}
// Slab entry k, its box inflated by D rho against the centre ray; (ix, iy, iz) = 1 / c (slab_rcp_v5).
RM_DEV bool cone_clears_slab_box_v5(const CullTables& T, const float2* aux, uint32_t k, float rho, float ix, float iy, float iz) {
    const float infl = aux[T.n_cone + k].y * rho;  // (|m|, D) both rounded up
    const float4 a = T.slab[3u * k], b = T.slab[3u * k + 1u];
    const float x1 = (a.x - infl) * ix, x2 = (b.x + infl) * ix, y1 = (a.y - infl) * iy, y2 = (b.y + infl) * iy;
    const float z1 = (a.z - infl) * iz, z2 = (b.z + infl) * iz;
    const float tn = fmax_(fmin_(x1, x2), fmax_(fmin_(y1, y2), fmin_(z1, z2)));
    const float tf = fmin_(fmax_(x1, x2), fmin_(fmax_(y1, y2), fmax_(z1, z2)));
    // infl must be a number for the comparison to mean anything (a dropped NaN would shrink the box)
    return infl < __uint_as_float(0x7F800000u) && !(tf >= fmax_(tn, 0.0f));
}
// Whether the tables clear every direction of a cone of rect_cone_v5 (cone_ok: what it returned).  mask (wave-uniform): the
// primitive mask of the tile the cone's rectangle lies in; V5_MASK_ALL tests every entry.
RM_DEV bool cone_misses_tables_v5(const CullTables& T, const float2* aux, const float (&cone)[4], bool cone_ok, uint32_t mask) {
    const float cx = cone[0], cy = cone[1], cz = cone[2], rho = cone[3];
    bool clear = cone_ok && *T.veto == 0u;  // a Plane (veto bit 1) leaves the tables unusable, not the cone
    if (mask != V5_MASK_ALL) {  // a mask in use: its set bits in ascending order; none: the pixel is clear without a table read
        for (uint32_t m = mask_cone_bits(mask, T.n_cone); m != 0u; m &= m - 1u)
            clear = clear && cone_clears_cone_entry_v5(T, aux, (uint32_t)__builtin_ctz(m), cx, cy, cz, rho);
        const uint32_t ms = mask_slab_bits(mask, T.n_cone);
        if (ms == 0u || __ballot(clear) == 0ull) return clear;
        const float ix = slab_rcp_v5(cx), iy = slab_rcp_v5(cy), iz = slab_rcp_v5(cz);
        for (uint32_t m = ms; m != 0u; m &= m - 1u) {
            const uint32_t k = (uint32_t)__builtin_ctz(m);
            if (__ballot(clear && !cone_clears_slab_sphere_v5(T, aux, k, cx, cy, cz, rho)) == 0ull) continue;
            clear = clear && cone_clears_slab_box_v5(T, aux, k, rho, ix, iy, iz);
            if (__ballot(clear) == 0ull) return false;
        }
        return clear;
    }
    for (uint32_t k = 0; k < T.n_cone; k++) {
        clear = clear && cone_clears_cone_entry_v5(T, aux, k, cx, cy, cz, rho);
        if ((k & 3u) == 3u && __ballot(clear) == 0ull) return false;
    }
    if (T.n_slab == 0u || __ballot(clear) == 0ull) return clear;
    const float ix = slab_rcp_v5(cx), iy = slab_rcp_v5(cy), iz = slab_rcp_v5(cz);
    for (uint32_t k = 0; k < T.n_slab; k++) {
        if (__ballot(clear && !cone_clears_slab_sphere_v5(T, aux, k, cx, cy, cz, rho)) == 0ull) continue;  // every still-clear pixel clears the bounding sphere
        clear = clear && cone_clears_slab_box_v5(T, aux, k, rho, ix, iy, iz);
        if (__ballot(clear) == 0ull) return false;
    }
    return clear;
}
// The same test entry by entry, lane = tile, for a program of at most 32 entries: `mask` gets bit k for cone entry k and bit
// n_cone + k for slab entry k iff the lane's cone does not provably clear the entry -- neither its bounding sphere nor, for a
// slab, its inflated box.  Returns what cone_misses_tables_v5(.., V5_MASK_ALL) returns in the same wave, bit for bit, and that
// is mask == 0 whenever cone_ok holds and nothing is vetoed: that function runs the box test of a slab for the whole wave as
// soon as ONE still-clear lane fails the sphere test, and a lane that is still clear then takes the box's verdict alone (it can
// be the stricter one: the box grows by D rho per axis, sqrt(3) D rho at its corners) -- so does its bit here.
RM_DEV bool tile_touch_mask_v5(const CullTables& T, const float2* aux, const float (&cone)[4], bool cone_ok, uint32_t& mask) {
    const float cx = cone[0], cy = cone[1], cz = cone[2], rho = cone[3];
    bool clear = cone_ok && *T.veto == 0u;
    uint32_t touched = 0u;
    for (uint32_t k = 0; k < T.n_cone; k++) {
        const bool ok = cone_clears_cone_entry_v5(T, aux, k, cx, cy, cz, rho);
        clear = clear && ok;
        touched |= ok ? 0u : 1u << k;
    }
    if (T.n_slab != 0u) {
        const float ix = slab_rcp_v5(cx), iy = slab_rcp_v5(cy), iz = slab_rcp_v5(cz);
        for (uint32_t k = 0; k < T.n_slab; k++) {
            const bool sphere_ok = cone_clears_slab_sphere_v5(T, aux, k, cx, cy, cz, rho);
            if (__ballot(!sphere_ok) == 0ull) continue;
            const bool wave_ran_box = __ballot(clear && !sphere_ok) != 0ull;
            const bool box_decides = clear && wave_ran_box;
            const bool box_ok = cone_clears_slab_box_v5(T, aux, k, rho, ix, iy, iz);
            const bool ok = box_decides ? box_ok : (sphere_ok || box_ok);
            clear = clear && ok;
            touched |= ok ? 0u : 1u << (T.n_cone + k);
        }
    }
    mask = touched;
    return clear;
}
// One pixel: the rectangle is its 4 x 4 grid of samples, spanned by samples (0,0), (3,0), (0,3), (3,3) (table entry 4 i + j of
// off, the table of the sixteen sample offsets).  mask: the primitive mask of the pixel's tile (V5_MASK_ALL: test every entry).
RM_DEV bool pixel_misses_scene_v5(const CullTables& T, const float2* aux, const float* m_proj, const float* m_view, const float* off,
                                  const V4& ro, float sx, float sy, float noise, uint32_t mask, float (&cone_out)[4], float (&corner)[4][3]) {
    const float px[2] = {sx, sx}, py[2] = {sy, sy}, ox[2] = {off[0], off[24]}, oy[2] = {off[1], off[7]};
    const bool cone_ok = rect_cone_v5(m_proj, m_view, ro, px, py, ox, oy, noise, cone_out, corner);
    return cone_misses_tables_v5(T, aux, cone_out, cone_ok, mask);
}

// The pixel test's own table, behind the miss-test tables: per cone / slab entry (|m|, |m| + bounding radius of the inflated
// box), both rounded up.  Whole workgroup, after the barrier behind cull_build_v5.
RM_DEV void pixel_aux_build_v5(const float4* t_cone, const float4* t_slab, uint32_t n_cone, uint32_t n_slab, float2* t_aux, uint32_t tid,
                               uint32_t n_threads) {
    const float up = 1.0f + 1.0e-6f;
    for (uint32_t k = tid; k < n_cone + n_slab; k += n_threads) {
        float4 m;
        float radius = 0.0f;
        if (k < n_cone) {
            m = t_cone[k];
        } else {
            const uint32_t j = k - n_cone;
            m = t_slab[3u * j + 2u];
            const float4 a = t_slab[3u * j], b = t_slab[3u * j + 1u];
            const float hx = b.x - a.x, hy = b.y - a.y, hz = b.z - a.z;  // full extents of the inflated box
            radius = 0.5f * __builtin_sqrtf(hx * hx + hy * hy + hz * hz) * up;
        }
        const float len = __builtin_sqrtf(m.x * m.x + m.y * m.y + m.z * m.z) * up;
        t_aux[k] = make_float2(len, (len + radius) * up);
    }
}

// The colour rules of a rectangle of sample positions whose rays all miss the scene.  corner[c]: pt_world.xyz - ro.xyz of its four
// extreme samples (rect_cone_v5); bx, by: upper bounds of |x|, |y| over the rectangle's positions.
//
// Sky: a sample whose ray points away from the floor plane (t <= 0 in wgsl:120-121) is black, and the sum of sixteen zeros is
// zero.  pt_world.y - ro.y is affine in the sample's screen position, so its sign over the rectangle is decided at the four
// corner samples up to rounding; with the camera above the plane (-1.5 - ro.y < 0), "all four corners point up by more than the
// rounding can move any sample" means dy > 0, t < 0 for all of them.  The margin is 1e-5 of `mag`, the sum of the absolute
// values of every term the two mat-vecs add up for the y component (each of the ~30 roundings on the way is <= 6e-8 of a
// partial sum, hence of mag; interior and corner values each move by that, the affine argument needs twice it).  Anything
// non-finite fails the comparison.
RM_DEV bool rect_sky_v5(const rm_uniforms& u, const V4& ro, const float (&corner)[4][3], float bx, float by, float& mag) {
    float lo = __uint_as_float(0x7F800000u);
#pragma unroll
    for (uint32_t c = 0; c < 4u; c++) {
        lo = corner[c][1] < lo ? corner[c][1] : lo;
        if (!(corner[c][1] == corner[c][1])) lo = corner[c][1];  // a NaN sticks and makes the test below false
    }
    mag = __builtin_fabsf(ro.y);
#pragma unroll
    for (int k = 0; k < 4; k++)  // |inv_view row y| . (|inv_proj| (|x|, |y|, 1, 1))
        mag += __builtin_fabsf(u.inv_view[1 + 4 * k]) * (((__builtin_fabsf(u.inv_proj[k]) * bx + __builtin_fabsf(u.inv_proj[k + 4]) * by) +
                                                          __builtin_fabsf(u.inv_proj[k + 8])) + __builtin_fabsf(u.inv_proj[k + 12]));
    return (-1.5f - ro.y) < 0.0f && lo > 1.0e-5f * mag;
}
// Floor, one checker cell for the whole rectangle.  With every sample ray pointing down (t > 0) the floor point of a sample is
// fx = o.x + C ex / ey, C = -1.5 - o.y (the normalisation cancels), a linear-fractional function of the sample's screen
// position: monotone along every segment where ey keeps its sign, so over the rectangle it stays between its values at the four
// corner samples.  If the interval those span -- widened by everything rounding can do to a sample's own fx: the mat-vec errors
// E (4e-6 of `mag`, per component) pushed through |C| / |ey| (E_x + |ex| E_y / |ey|), once for the corners and once for the
// sample, the approximate reciprocal used here and the five roundings of the sample's own chain -- rounds to ONE integer after
// the +0.5 of wgsl:124 (rint is monotone), and the same holds for z, all samples carry the same checker bit `code`, and each
// pixel is the sum of sixteen equal gamma values.  mag: as rect_sky_v5 left it.
RM_DEV bool rect_cell_v5(const rm_uniforms& u, const V4& ro, const float (&corner)[4][3], float bx, float by, float mag, int& code) {
    const float Cf = -1.5f - ro.y;  // as shade_floor computes it
    float ex[4], eyc[4], ez[4], ey_hi = -__uint_as_float(0x7F800000u), ax_hi = 0.0f, az_hi = 0.0f;
#pragma unroll
    for (uint32_t c = 0; c < 4u; c++) {
        ex[c] = corner[c][0]; eyc[c] = corner[c][1]; ez[c] = corner[c][2];
        ey_hi = eyc[c] > ey_hi ? eyc[c] : ey_hi;
        if (!(eyc[c] == eyc[c])) ey_hi = eyc[c];
        ax_hi = fmax_(ax_hi, __builtin_fabsf(ex[c]));
        az_hi = fmax_(az_hi, __builtin_fabsf(ez[c]));
    }
    float mag_x = __builtin_fabsf(ro.x), mag_z = __builtin_fabsf(ro.z);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float pvk = ((__builtin_fabsf(u.inv_proj[k]) * bx + __builtin_fabsf(u.inv_proj[k + 4]) * by) + __builtin_fabsf(u.inv_proj[k + 8])) +
                          __builtin_fabsf(u.inv_proj[k + 12]);
        mag_x += __builtin_fabsf(u.inv_view[0 + 4 * k]) * pvk;
        mag_z += __builtin_fabsf(u.inv_view[2 + 4 * k]) * pvk;
    }
    const float Ey = 4.0e-6f * mag, Ex = 4.0e-6f * mag_x, Ez = 4.0e-6f * mag_z;
    const float my = -ey_hi - 2.0f * Ey;  // every sample's |ey| is at least this
    bool uniform = Cf < -1.0e-20f && my > 0.0f && ey_hi < -4.0f * Ey;
    const float inv_my = __builtin_amdgcn_rcpf(my) * 1.00001f, absC = -Cf;
    float gx_lo = __uint_as_float(0x7F800000u), gx_hi = -gx_lo, gz_lo = gx_lo, gz_hi = -gx_lo;
#pragma unroll
    for (uint32_t c = 0; c < 4u; c++) {
        const float r = __builtin_amdgcn_rcpf(eyc[c]);
        const float gx = ex[c] * r, gz = ez[c] * r;
        gx_lo = fmin_(gx_lo, gx); gx_hi = fmax_(gx_hi, gx);
        gz_lo = fmin_(gz_lo, gz); gz_hi = fmax_(gz_hi, gz);
        uniform = uniform && gx == gx && gz == gz;  // (v_min / v_max drop a NaN)
    }
    // C < 0: the interval of fx - o.x is [C gx_hi, C gx_lo]
    const float dx_lo = Cf * gx_hi, dx_hi = Cf * gx_lo, dz_lo = Cf * gz_hi, dz_hi = Cf * gz_lo;
    const float dev_x = fmax_(__builtin_fabsf(dx_lo), __builtin_fabsf(dx_hi)), dev_z = fmax_(__builtin_fabsf(dz_lo), __builtin_fabsf(dz_hi));
    const float del_x = 4.0f * (absC * inv_my) * (Ex + ((ax_hi + Ex) * inv_my) * Ey) + 2.0e-5f * ((1.0f + __builtin_fabsf(ro.x)) + dev_x);
    const float del_z = 4.0f * (absC * inv_my) * (Ez + ((az_hi + Ez) * inv_my) * Ey) + 2.0e-5f * ((1.0f + __builtin_fabsf(ro.z)) + dev_z);
    const float nx = __builtin_rintf(((ro.x + dx_lo) - del_x) + 0.5f), nz = __builtin_rintf(((ro.z + dz_lo) - del_z) + 0.5f);
    uniform = uniform && nx == __builtin_rintf(((ro.x + dx_hi) + del_x) + 0.5f) && nz == __builtin_rintf(((ro.z + dz_hi) + del_z) + 0.5f);
    code = (__float2int_rz(nx) ^ __float2int_rz(nz)) & 1;  // as shade_floor: saturating, wgsl:124-126
    return uniform;
}

// Verdict bits of a tile (tile_verdict_v5): the tables clear it / all its samples are sky / all are in one checker cell, whose
// bit is V5_TILE_CODE.  Settled here: CLEAR and (SKY or CELL).
constexpr uint32_t V5_TILE_CLEAR = 1u, V5_TILE_SKY = 2u, V5_TILE_CELL = 4u, V5_TILE_CODE = 8u;
// One lane, one tile (tile_x, tile_y) of eight consecutive frame rows from strip-local row 8 tile_y on (see the header above).
// tables: the miss-test tables are staged; all_miss: no ray can hit anything (max_iter = 0).  off: the sixteen sample offsets.
// mask: the tile's primitive mask (tile_touch_mask_v5) where it is exact information -- the tables were consulted and are
// usable, the cone is, the program has at most 32 entries --, else V5_MASK_ALL.
RM_DEV uint32_t tile_verdict_v5(const RmLaunch& L, const rm_uniforms& u, const V4& ro, const CullTables& T, const float2* aux, const float* off,
                                bool tables, bool all_miss, uint32_t tile_x, uint32_t tile_y, float (&cone)[4], uint32_t& mask) {
    const uint32_t row = rm_global_row(L, tile_y * 8u);
    const float px[2] = {screen_x(tile_x * 8u, L.W), screen_x(tile_x * 8u + 7u, L.W)};
    const float py[2] = {screen_y(row, L.H), screen_y(row + 7u, L.H)};
    // samples 0 and 3 carry the extreme offsets, in an order the viewport's signs decide
    const float ox[2] = {fmin_(off[0], off[24]), fmax_(off[0], off[24])}, oy[2] = {fmax_(off[1], off[7]), fmin_(off[1], off[7])};
    float corner[4][3];
    const bool cone_ok = rect_cone_v5(u.inv_proj, u.inv_view, ro, px, py, ox, oy, cone_noise_v5(u, ro, L.W, L.H), cone, corner);
    bool clear = cone_ok && all_miss;
    mask = V5_MASK_ALL;
    if (!all_miss && tables) {
        if (T.n_cone + T.n_slab <= 32u) {  // (wave-uniform)
            uint32_t touched;
            clear = tile_touch_mask_v5(T, aux, cone, cone_ok, touched);
            if (cone_ok && *T.veto == 0u) mask = touched;
        } else {
            clear = cone_misses_tables_v5(T, aux, cone, cone_ok, V5_MASK_ALL);
        }
    }
    float bx = 0.0f, by = 0.0f;
#pragma unroll
    for (int a = 0; a < 2; a++) {
        bx = fmax_(bx, __builtin_fabsf(px[a] + ox[a]));
        by = fmax_(by, __builtin_fabsf(py[a] + oy[a]));
    }
    float mag;
    int code = 0;
    const bool sky = rect_sky_v5(u, ro, corner, bx, by, mag);
    const bool cell = !sky && rect_cell_v5(u, ro, corner, bx, by, mag, code);
    // (a NaN offset or position: v_min / v_max drop it, but it reaches the corners and fails the cone)
    // A block that maps the tile's 8 x 8 pixels onto ONE direction (a singular inv_proj: all zeros sends every sample to -ro) is no
    // camera: the four corners coincide, the rules above would hold trivially, and nothing is settled per tile -- the per-pixel
    // path draws such a frame.
    bool spread = false;
#pragma unroll
    for (uint32_t c = 1; c < 4u; c++) spread = spread || corner[c][0] != corner[0][0] || corner[c][1] != corner[0][1] || corner[c][2] != corner[0][2];
    if (!spread) {
        mask = V5_MASK_ALL;
        return 0u;
    }
    return (clear ? V5_TILE_CLEAR : 0u) | (sky ? V5_TILE_SKY : 0u) | (cell ? V5_TILE_CELL | (code ? V5_TILE_CODE : 0u) : 0u);
}

// The miss-test tables of the launch's program for rays from `ro`, staged in the workgroup's dynamic LDS (rml::CullLds) by all
// its n_threads threads; ends with a barrier.  The pre-pass and the culling self-tests stage them through this one function.
//   off   nullptr, or [16][2]: the screen offsets of the AA samples under `u` are computed alongside
//   aux   nullptr, or where to return the rows [n_cone + n_slab] (|m|, |m| + bounding radius) of the pixel and tile tests
RM_DEV CullTables stage_cull_tables(const RmLaunch& L, const V4& ro, uint32_t* smem, const rm_uniforms* u, float* off, const float2** aux,
                                    uint32_t tid, uint32_t n_threads) {
    const rml::CullLds lds(L.n_cone, L.n_slab, aux != nullptr);
    uint32_t* s_veto = lds_at<uint32_t>(smem, lds.veto);
    float4* t_cone = lds_at<float4>(smem, lds.cone);
    float4* t_slab = lds_at<float4>(smem, lds.slab);
    const bool tables = (L.flags & 1u) != 0u;
    if (tid == 0u) *s_veto = 0u;
    if (off && tid < 16u) sample_offset(*u, tid >> 2, tid & 3u, off[2u * tid], off[2u * tid + 1u]);
    __syncthreads();
    if (tables)
        for (uint32_t k = tid; k < L.n_rec; k += n_threads) cull_build_v5(L.prog[k], ro, L.min_dist, L.smooth_slack, t_cone, t_slab, s_veto, L.bounds);
    __syncthreads();
    if (aux) {
        float2* t_aux = lds_at<float2>(smem, lds.aux);
        if (tables) pixel_aux_build_v5(t_cone, t_slab, L.n_cone, L.n_slab, t_aux, tid, n_threads);
        __syncthreads();
        *aux = t_aux;
    }
    return CullTables{t_cone, t_slab, s_veto, L.n_cone, L.n_slab};
}

__global__ __launch_bounds__(64 * V5_PRE_TILES) void rm_tile_pre_v5(RmLaunch L, uint32_t* cost, uint32_t* masks, uint32_t n_tiles) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    rm_uniforms u = L.u;
    if (L.frames) u = L.frames[blockIdx.z];
    const V4 ro = matvec(u.inv_view, 0.0f, 0.0f, 0.0f, 1.0f);
    const bool tables = (L.flags & 1u) != 0u;
    __shared__ float s_off[32];  // screen offsets of the 16 AA samples: the same for every pixel, computed once
    __shared__ float s_sxy[V5_PRE_TILES][128];          // per wave: pixel centres, sample codes and the list of the pixels that
    __shared__ uint8_t s_code[V5_PRE_TILES][64 * 16];   // need them, for the sample-parallel finish of a clear tile (below)
    __shared__ uint8_t s_list[V5_PRE_TILES][64];
    __shared__ uint8_t s_verdict[V5_PRE_BLOCK];  // per tile of the block: tile_verdict_v5 if it settles the tile, else 0
    __shared__ uint32_t s_mask[V5_PRE_BLOCK];    // per tile of the block: its primitive mask (also written to masks[], for the march kernel)
    __shared__ uint32_t s_claim;                 // next tile of the block to hand out
    if (tid == 0u) s_claim = 0u;
    const float2* t_aux;
    const CullTables cullt = stage_cull_tables(L, ro, smem, &u, s_off, &t_aux, tid, 64u * V5_PRE_TILES);
    const uint32_t* s_veto = cullt.veto;
    const uint32_t tiles_x = (L.W + 7u) / 8u;
    const float cone_noise = cone_noise_v5(u, ro, L.W, L.H);
  auto do_tile = [&](uint32_t tile, uint32_t tile_mask) {  // (whole wave; no barrier inside; tile_mask wave-uniform)
    const uint32_t tile_x = tile % tiles_x, tile_y = tile / tiles_x;
    const uint32_t tx = tile_x * 8u + (lane & 7u), ty = tile_y * 8u + (lane >> 3);
    const uint32_t px = tx < L.W ? tx : L.W - 1u, ry = ty < L.rows ? ty : L.rows - 1u;
    const float sx = screen_x(px, L.W), sy = screen_y(rm_global_row(L, ry), L.H);
    // the two matrices in vector registers (32 of them): as scalar operands every multiply of the mat-vecs -- the four corner rays
    // here, the sixteen sample rays of the finishing loop -- would issue at half rate
    float mp[16], mv[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        mp[k] = u.inv_proj[k]; mv[k] = u.inv_view[k];
        asm volatile("" : "+v"(mp[k]), "+v"(mv[k]));
    }
    bool clear;
    float corner[4][3];  // pt_world.xyz - ro.xyz of the pixel's four corner samples
    if (L.max_iter == 0u || !tables) {
        clear = L.max_iter == 0u;  // no march step is ever taken: every ray is a miss (wgsl:92); without tables nothing is known
#pragma unroll
        for (uint32_t c = 0; c < 4u; c++) {
            const uint32_t s = ((c & 1u) * 3u) * 4u + (c >> 1) * 3u;
            gen_ray_unnormalized_at(mp, mv, ro, sx, sy, s_off[2u * s], s_off[2u * s + 1u], corner[c][0], corner[c][1], corner[c][2]);
        }
    } else {
        float cone[4];
        clear = pixel_misses_scene_v5(cullt, t_aux, mp, mv, s_off, ro, sx, sy, cone_noise, tile_mask, cone, corner);
        // a program that blends: the pixels the inflated bounds could not clear get the program run on lower bounds of its
        // leaves over the pixel's cone ("Miss test on lower bounds"; the march kernel repeats it per ray for what is left)
        const float bound_scale = bound_scale_prepass_v5(L, ro);
        if ((L.flags & 32u) && (*s_veto & 1u) == 0u && bound_scale < 1.0e12f && __ballot(!clear && cone[3] == cone[3]) != 0ull) {
            const ProgSmem prog{L.prog};  // wave-uniform addresses: scalar loads
            auto load_record = [&](uint32_t i, uint32_t& op, float (&p)[7]) { prog.load(i, op, p); };
            const bool by_bounds = ray_misses_by_bounds_v5<true>(load_record, L.n_rec, ro, cone[0], cone[1], cone[2], L.min_dist, bound_scale, cone[3]);
            clear = clear || (cone[3] == cone[3] && by_bounds);
        }
    }
    const uint32_t pending = (uint32_t)__popcll(__ballot(!clear));
    if (lane == 0u) cost[(size_t)blockIdx.z * n_tiles + tile] = pending;  // 0 = finished here
    if (pending != 0u) return;
    // this pixel's sixteen samples provably share one colour code (rect_sky_v5 / rect_cell_v5 on the pixel's 4 x 4 grid):
    // -1 black (sky), 0 / 1 the checker bit.  A tile whose 64 pixels are all sky writes zeros and skips the loop below; one whose
    // pixels are each sky or one cell skips the sample rays: what remains for it are the pixels a cell edge crosses, the horizon
    // and the far floor.
    const float bx = __builtin_fabsf(sx) + __builtin_fabsf(s_off[0]), by = __builtin_fabsf(sy) + __builtin_fabsf(s_off[1]);  // sample (0, 0) has the largest offsets
    float mag;
    const bool sky = rect_sky_v5(u, ro, corner, bx, by, mag);
    if (__ballot(!sky) == 0ull) {
        if (tx < L.W && ty < L.rows) store_pixel(L, blockIdx.z, (size_t)ty * L.W + tx, 0.0f, 0.0f, 0.0f);  // 0 / 16 = 0 (wgsl:73-75)
        return;
    }
    int cell_code;
    const bool uniform = rect_cell_v5(u, ro, corner, bx, by, mag, cell_code);
    const bool known = sky || uniform;
    const int known_code = sky ? -1 : cell_code;
    // The sample loop.  Everything that does not depend on the pixel is taken out of it: the sample offsets (two divisions each)
    // come from the table, the matrices sit in vector registers, and the gamma-corrected colour of a sample is one of three
    // values -- black, or the checker colour for bit 0 / 1 (wgsl:127) -- whose square roots are taken once, by the same
    // expressions.
    float gamma_rg[2], gamma_b[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const float g = 0.2f * (float)c;
        gamma_rg[c] = __builtin_sqrtf(0.1f + g);
        gamma_b[c] = __builtin_sqrtf(0.2f + g);
    }
    auto gamma_of = [&](int c, float& rg, float& b) {
        rg = c < 0 ? 0.0f : (c ? gamma_rg[1] : gamma_rg[0]);  // sqrt(0) = 0 (wgsl:130)
        b = c < 0 ? 0.0f : (c ? gamma_b[1] : gamma_b[0]);
    };
    float tr = 0.0f, tg = 0.0f, tb = 0.0f;
    const unsigned long long need = __ballot(!known);  // pixels whose samples have to be looked at one by one
    const uint32_t n_need = (uint32_t)__popcll(need);
    if (n_need <= 24u) {
        // Few such pixels (a checker edge crossing the tile): their samples -- 16 n_need of them -- are spread over the 64
        // lanes, 64 per pass instead of one sample of all 64 pixels per pass; each sample's colour code goes to LDS and the
        // pixel's lane then adds its sixteen gamma values in the reference order.  Same functions, same sums.
        float* w_sxy = s_sxy[wave];
        uint8_t* w_code = s_code[wave];
        uint8_t* w_list = s_list[wave];
        w_sxy[lane] = sx; w_sxy[64u + lane] = sy;
        if (!known) w_list[lane_rank(need)] = (uint8_t)lane;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (uint32_t base = 0u; base < 16u * n_need; base += 64u) {
            const uint32_t item = base + lane, q = item >> 4, s = item & 15u;
            const uint32_t pl = w_list[q < n_need ? q : 0u];
            float dx, dy, dz;
            gen_ray_at<true>(mp, mv, ro, w_sxy[pl], w_sxy[64u + pl], s_off[2u * s], s_off[2u * s + 1u], dx, dy, dz);
            const int c = shade_floor(ro.y, ro.x, ro.z, dx, dy, dz);  // wgsl:117-130
            if (q < n_need) w_code[pl * 16u + s] = (uint8_t)(c + 1);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (uint32_t s = 0; s < 16u; s++) {  // reference order: wgsl:44-45, 68-69
            const int c = known ? known_code : (int)w_code[lane * 16u + s] - 1;
            float rg, b;
            gamma_of(c, rg, b);
            tr += rg;
            tg += rg;
            tb += b;
        }
    } else {
        for (uint32_t s = 0; s < 16u; s++) {  // reference order: wgsl:44-45, 68-69
            float dx, dy, dz;
            gen_ray_at<true>(mp, mv, ro, sx, sy, s_off[2u * s], s_off[2u * s + 1u], dx, dy, dz);
            const int c = shade_floor(ro.y, ro.x, ro.z, dx, dy, dz);  // wgsl:117-130
            float rg, b;
            gamma_of(c, rg, b);
            tr += rg;
            tg += rg;
            tb += b;
        }
    }
    if (tx < L.W && ty < L.rows) {
        store_pixel(L, blockIdx.z, (size_t)ty * L.W + tx, tr / 16.0f, tg / 16.0f, tb / 16.0f);  // wgsl:73-75
    }
  };
    // Tile verdicts, lane = tile; without tables nothing is known unless no ray can hit (do_tile decides the same way), and
    // a tile's rows must be consecutive frame rows
    const uint32_t first_tile = blockIdx.x * V5_PRE_BLOCK;
    if (tid < V5_PRE_BLOCK) {
        uint32_t v = 0u, mask = V5_MASK_ALL;
        if ((tables || L.max_iter == 0u) && L.strip_rows % 8u == 0u) {
            const uint32_t tile = first_tile + tid < n_tiles ? first_tile + tid : n_tiles - 1u;
            float cone[4];
            v = tile_verdict_v5(L, u, ro, cullt, t_aux, s_off, tables, L.max_iter == 0u, tile % tiles_x, tile / tiles_x, cone, mask);
            if (!(v & V5_TILE_CLEAR) || !(v & (V5_TILE_SKY | V5_TILE_CELL))) v = 0u;
        }
        s_verdict[tid] = (uint8_t)v;
        s_mask[tid] = mask;
        if (first_tile + tid < n_tiles) masks[(size_t)blockIdx.z * n_tiles + first_tile + tid] = mask;
    }
    __syncthreads();
    for (;;) {
        uint32_t t = 0u;
        if (lane == 0u) t = atomicAdd(&s_claim, 1u);
        t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
        if (t >= V5_PRE_BLOCK || first_tile + t >= n_tiles) break;
        const uint32_t tile = first_tile + t, v = s_verdict[t];
        if (v == 0u) {
            do_tile(tile, (uint32_t)__builtin_amdgcn_readfirstlane((int)s_mask[t]));
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the wave's LDS scratch is reused by its next tile
            continue;
        }
        // settled: one constant for the tile's 64 pixels, added up as do_tile's sample loop adds a pixel's sixteen equal values
        float tr = 0.0f, tb = 0.0f;
        if (v & V5_TILE_CELL) {
            const float g = 0.2f * (float)((v & V5_TILE_CODE) ? 1 : 0);
            const float rg = __builtin_sqrtf(0.1f + g), b = __builtin_sqrtf(0.2f + g);
            for (uint32_t s = 0; s < 16u; s++) {
                tr += rg;
                tb += b;
            }
        }
        const uint32_t tx = (tile % tiles_x) * 8u + (lane & 7u), ty = (tile / tiles_x) * 8u + (lane >> 3);
        if (lane == 0u) cost[(size_t)blockIdx.z * n_tiles + tile] = 0u;
        if (tx < L.W && ty < L.rows) store_pixel(L, blockIdx.z, (size_t)ty * L.W + tx, tr / 16.0f, tr / 16.0f, tb / 16.0f);  // wgsl:73-75
    }
}
#endif

// Work list of one frame (blockIdx.x = frame): ids of the tiles with cost > 0, by descending cost
// when `balance` is set.  Also resets the persistent kernel's cursor.
#if !defined(RM_JIT_TU)  // not part of a specialised translation unit (rm_jit.h)
// With `prev` (what the previous draw of the same shape measured per tile) the key of a tile that was marched then is
// its duration on a 4-steps-per-octave log scale, so that the LONGEST tiles are dispatched first and the kernel ends
// on its shortest ones; a tile without a measurement keeps its pending-pixel count (64 for a fully covered tile, i.e.
// it is treated as heavy).  The order only affects when a tile is rendered, never its pixels.
RM_DEV uint32_t duration_key(uint32_t ticks) {  // 1..64; 64 ticks (0.64 us) -> 1, doubling adds 4
    if (ticks < 64u) return 1u;
    const uint32_t lz = 31u - (uint32_t)__builtin_clz(ticks);
    const uint32_t q = 4u * lz + ((ticks >> (lz - 2u)) & 3u) - 23u;
    return q > 64u ? 64u : q;
}
__global__ __launch_bounds__(1024) void rm_tile_sort_v5(RmLaunch L, const uint32_t* cost, uint32_t* order, uint32_t* counters,
                                                        uint32_t n_tiles, uint32_t balance, const uint32_t* prev) {
    __shared__ uint32_t hist[65], base[65];
    __shared__ float f0_spill[(32 + 3 * RM_MAX_XFORM_DEPTH) * 64];
    const uint32_t tid = threadIdx.x;
    // f0 = map_scene(ro): the first march step every ray of this frame shares (see rm_render_v5_body).  The
    // interpreter with the correctly rounded library sqrt gives the same bits as every kernel's evaluation.
    if (tid >= 960u) {  // the last wave; it has the least to do in the loops below
        rm_uniforms u = L.u;
        if (L.frames) u = L.frames[blockIdx.x];
        const V4 ro = matvec(u.inv_view, 0.0f, 0.0f, 0.0f, 1.0f);
        ProgSmem prog;
        prog.base = L.prog;
        const float qx[1] = {ro.x}, qy[1] = {ro.y}, qz[1] = {ro.z};
        float v[1];
        SqrtGuard tiny;
        map_scene_multi<1, false, ProgSmem, true>(prog, L.n_rec, f0_spill + (tid & 63u), L.max_dist, qx, qy, qz, v, tiny, L.value_spill_depth);
        if (tid == 960u) counters[4u * blockIdx.x + 2u] = __float_as_uint(v[0]);
    }
    const uint32_t* c = cost + (size_t)blockIdx.x * n_tiles;
    const uint32_t* pm = prev ? prev + (size_t)blockIdx.x * n_tiles : nullptr;
    uint32_t* o = order + (size_t)blockIdx.x * n_tiles;
    // keys of tiles i0 + tid + 1024 j, j = 0..7: the loads of a batch are issued together (one workgroup walks the whole list;
    // with one dependent load per trip the two passes below were 32 round trips to L2 each, 35 us for a 1080p frame)
    constexpr uint32_t B = 8u;
    auto keys_of = [&](uint32_t i0, uint32_t (&v)[B]) {
        uint32_t t[B];
#pragma unroll
        for (uint32_t j = 0; j < B; j++) {
            const uint32_t i = i0 + j * 1024u + tid;
            v[j] = i < n_tiles ? c[i] : 0u;
            t[j] = (pm && i < n_tiles) ? pm[i] : 0u;
        }
#pragma unroll
        for (uint32_t j = 0; j < B; j++)
            if (v[j] != 0u && t[j] != 0u) v[j] = duration_key(t[j]);
    };
    if (tid < 65u) hist[tid] = 0u;
    __syncthreads();
    // bucket 0 = heaviest (cost 64) ... bucket 63 = cost 1; cost 0 (finished in the pre-pass) is dropped
    auto bucket = [&](uint32_t v) { return balance ? 64u - (v < 64u ? v : 64u) : 0u; };
    for (uint32_t i0 = 0; i0 < n_tiles; i0 += 1024u * B) {
        uint32_t vs[B];
        keys_of(i0, vs);
#pragma unroll
        for (uint32_t j = 0; j < B; j++) {
            const uint32_t v = vs[j];
            // most active tiles have the same cost (64): count those once per wave, not once per lane
            const unsigned long long heavy = __ballot(v != 0u && bucket(v) == 0u);
            if (heavy != 0ull && (tid & 63u) == (uint32_t)__builtin_ctzll(heavy)) atomicAdd(&hist[0], (uint32_t)__popcll(heavy));
            if (v != 0u && bucket(v) != 0u) atomicAdd(&hist[bucket(v)], 1u);
        }
    }
    __syncthreads();
    if (tid == 0u) {
        uint32_t acc = 0u;
        if (balance == 2u) {  // partially covered tiles (silhouettes: that is where the rays that never converge are) first
            for (uint32_t b = 1; b < 65u; b++) { base[b] = acc; acc += hist[b]; }
            base[0] = acc;
            acc += hist[0];
        } else {
            for (uint32_t b = 0; b < 65u; b++) { base[b] = acc; acc += hist[b]; }
        }
        counters[4u * blockIdx.x] = acc;      // tiles on the work list
        counters[4u * blockIdx.x + 1u] = 0u;  // cursor
    }
    __syncthreads();
    for (uint32_t i0 = 0; i0 < n_tiles; i0 += 1024u * B) {
        uint32_t vs[B];
        keys_of(i0, vs);
#pragma unroll
        for (uint32_t j = 0; j < B; j++) {
            const uint32_t i = i0 + j * 1024u + tid;
            const uint32_t v = vs[j];
            const bool is_heavy = v != 0u && bucket(v) == 0u;
            const unsigned long long heavy = __ballot(is_heavy);
            uint32_t pos0 = 0u;
            if (heavy != 0ull) {
                const int leader = __builtin_ctzll(heavy);
                if ((int)(tid & 63u) == leader) pos0 = atomicAdd(&base[0], (uint32_t)__popcll(heavy));
                pos0 = __shfl(pos0, leader);
            }
            if (is_heavy) o[pos0 + lane_rank(heavy)] = i;
            else if (v != 0u) o[atomicAdd(&base[bucket(v)], 1u)] = i;
        }
    }
}
#endif

// ---- Self-tests of the culling decisions (rm_selftest_cull_*; tests/test_gpu_cull_bounds.py) ------------------------------------
// The device functions above on inputs the caller chooses, with the launch a draw of the context's program would get and the
// tables staged in LDS by the function that stages them for rm_tile_pre_v5, stage_cull_tables.  (They stand here, not next to
// rm_selftest_wave_kernel: they need the functions defined since.)
#if !defined(RM_JIT_TU)
// LDS: rml::CullLds, with the aux rows for the pixel and tile probes.  One wave per workgroup.
// Rays: out_flags[i] bit 0 the verdict of ray_misses_scene_v5 (false without culling), bit 1 the tables were usable (culling on, no
// veto), bit 2 the walk on lower bounds applies, bit 3 its verdict, bits 8.. the veto word; out_bound[i] the walk's bound (NaN
// when it does not apply).
__global__ __launch_bounds__(64) void rm_selftest_cull_rays_kernel(RmLaunch L, V4 ro, const float* dirs, uint32_t n, uint32_t* out_flags,
                                                                   float* out_bound) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t tid = threadIdx.x;
    const bool tables = (L.flags & 1u) != 0u;
    const CullTables cullt = stage_cull_tables(L, ro, smem, nullptr, nullptr, nullptr, tid, 64u);
    const uint32_t i = blockIdx.x * 64u + tid, j = i < n ? i : n - 1u;
    const float gx = dirs[3u * j], gy = dirs[3u * j + 1u], gz = dirs[3u * j + 2u];
    const uint32_t veto = *cullt.veto;
    const bool clear = tables && ray_misses_scene_v5(cullt, V5_MASK_ALL, gx, gy, gz);
    const float bound_scale = bound_scale_march_v5(L, ro);
    const bool walk = tables && (L.flags & 32u) && (veto & 1u) == 0u && bound_scale < 1.0e12f;
    float acc = __uint_as_float(0x7FC00000u);
    bool by_bounds = false;
    if (walk) {
        const ProgSmem prog{L.prog};  // wave-uniform addresses: scalar loads
        auto load_record = [&](uint32_t r, uint32_t& op, float (&p)[7]) { prog.load(r, op, p); };
        acc = ray_bound_v5<false>(load_record, L.n_rec, ro, gx, gy, gz, bound_scale);
        by_bounds = ray_misses_by_bounds_v5<false>(load_record, L.n_rec, ro, gx, gy, gz, L.min_dist, bound_scale);
    }
    if (i < n) {
        out_flags[i] = (clear ? 1u : 0u) | ((tables && veto == 0u) ? 2u : 0u) | (walk ? 4u : 0u) | (by_bounds ? 8u : 0u) | (veto << 8);
        out_bound[i] = acc;
    }
}
// Pixels of a W x H frame (L.W, L.H) under the context's uniforms: out[8 i + 0..3] the cone (c, rho) of pixel_misses_scene_v5
// (rho = NaN: not usable), [4] the CONE walk's bound (NaN when it does not apply), [5] flags as an integer: bit 0 the verdict of
// pixel_misses_scene_v5, bit 1 the tables were usable, bit 2 the CONE walk applies, bit 3 its verdict; [6], [7] zero.
__global__ __launch_bounds__(64) void rm_selftest_cull_pixels_kernel(RmLaunch L, const uint32_t* xy, uint32_t n, float* out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    __shared__ float s_off[32];
    const uint32_t tid = threadIdx.x;
    const rm_uniforms u = L.u;
    const V4 ro = matvec(u.inv_view, 0.0f, 0.0f, 0.0f, 1.0f);
    const bool tables = (L.flags & 1u) != 0u;
    const float2* t_aux;
    const CullTables cullt = stage_cull_tables(L, ro, smem, &u, s_off, &t_aux, tid, 64u);
    const uint32_t i = blockIdx.x * 64u + tid, j = i < n ? i : n - 1u;
    const float sx = screen_x(xy[2u * j], L.W), sy = screen_y(rm_global_row(L, xy[2u * j + 1u]), L.H);
    float mp[16], mv[16];
#pragma unroll
    for (int k = 0; k < 16; k++) { mp[k] = u.inv_proj[k]; mv[k] = u.inv_view[k]; }
    const float nan = __uint_as_float(0x7FC00000u), cone_noise = cone_noise_v5(u, ro, L.W, L.H);
    float cone[4] = {nan, nan, nan, nan}, corner[4][3], acc = nan;
    bool clear = false, walk = false, by_bounds = false;
    const uint32_t veto = *cullt.veto;
    if (tables) {
        clear = pixel_misses_scene_v5(cullt, t_aux, mp, mv, s_off, ro, sx, sy, cone_noise, V5_MASK_ALL, cone, corner);
        const float bound_scale = bound_scale_prepass_v5(L, ro);
        walk = (L.flags & 32u) && (veto & 1u) == 0u && bound_scale < 1.0e12f && cone[3] == cone[3];
        if (__ballot(walk) != 0ull) {
            const ProgSmem prog{L.prog};
            auto load_record = [&](uint32_t r, uint32_t& op, float (&p)[7]) { prog.load(r, op, p); };
            const float b = ray_bound_v5<true>(load_record, L.n_rec, ro, cone[0], cone[1], cone[2], bound_scale, cone[3]);
            const bool v = ray_misses_by_bounds_v5<true>(load_record, L.n_rec, ro, cone[0], cone[1], cone[2], L.min_dist, bound_scale, cone[3]);
            if (walk) { acc = b; by_bounds = v; }
        }
    }
    if (i < n) {
        float* o = out + 8u * (size_t)i;
        o[0] = cone[0]; o[1] = cone[1]; o[2] = cone[2]; o[3] = cone[3]; o[4] = acc;
        o[5] = __uint_as_float((clear ? 1u : 0u) | ((tables && veto == 0u) ? 2u : 0u) | (walk ? 4u : 0u) | (by_bounds ? 8u : 0u));
        o[6] = 0.0f; o[7] = 0.0f;
    }
}
// Tiles xy[2 i] = (tile_x, tile_y) of a W x H frame (L.W, L.H) under the context's uniforms, as the pre-pass classifies them, lane
// = tile: out[8 i + 0..3] the cone (c, rho) of the tile's 32 x 32 sample directions (rho = NaN: not usable), [4] the checker bit
// of a one-cell tile (else 0), [5] flags as an integer: bit 0 the tables clear the tile, bit 1 all its samples are sky, bit 2 all
// are in one checker cell, bit 3 the tables were usable; [6] the tile's primitive mask as an integer (V5_MASK_ALL when it is
// not in use), [7] the number of table entries n_cone + n_slab as an integer.
__global__ __launch_bounds__(64) void rm_selftest_cull_tiles_kernel(RmLaunch L, const uint32_t* xy, uint32_t n, float* out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    __shared__ float s_off[32];
    const uint32_t tid = threadIdx.x;
    const rm_uniforms u = L.u;
    const V4 ro = matvec(u.inv_view, 0.0f, 0.0f, 0.0f, 1.0f);
    const bool tables = (L.flags & 1u) != 0u;
    const float2* t_aux;
    const CullTables cullt = stage_cull_tables(L, ro, smem, &u, s_off, &t_aux, tid, 64u);
    const uint32_t i = blockIdx.x * 64u + tid, j = i < n ? i : n - 1u;
    float cone[4];
    uint32_t mask;
    const uint32_t v = tile_verdict_v5(L, u, ro, cullt, t_aux, s_off, tables, L.max_iter == 0u, xy[2u * j], xy[2u * j + 1u], cone, mask);
    if (L.strip_rows % 8u != 0u) mask = V5_MASK_ALL;  // (as rm_tile_pre_v5: no verdicts on tiles whose rows are not consecutive)
    if (i < n) {
        float* o = out + 8u * (size_t)i;
        o[0] = cone[0]; o[1] = cone[1]; o[2] = cone[2]; o[3] = cone[3];
        o[4] = (v & V5_TILE_CODE) ? 1.0f : 0.0f;
        o[5] = __uint_as_float(((v & V5_TILE_CLEAR) ? 1u : 0u) | ((v & V5_TILE_SKY) ? 2u : 0u) | ((v & V5_TILE_CELL) ? 4u : 0u) |
                               ((tables && *cullt.veto == 0u) ? 8u : 0u));
        o[6] = __uint_as_float(mask); o[7] = __uint_as_float(L.n_cone + L.n_slab);
    }
}
// Waves: pos[(3 w + k) * 64 + lane] coordinate k of wave w's lane, thr[64 w + lane], live[w] the mask of its live lanes (not 0);
// out[w] the mask of wave_cull_lattice or wave_cull_blend, by the program's unit_mode (not RM_UNITS_NONE).  LDS: the unit table.
__global__ __launch_bounds__(64) void rm_selftest_cull_waves_kernel(RmLaunch L, V4 ro, const float* pos, const float* thr, const unsigned long long* live,
                                                                    float extra_margin, unsigned long long* out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t lane = threadIdx.x, w = blockIdx.x;
    stage_units(smem, L.prog + L.n_rec, L.n_grp, lane, 64u);
    __syncthreads();
    const float x = pos[(3u * w) * 64u + lane], y = pos[(3u * w + 1u) * 64u + lane], z = pos[(3u * w + 2u) * 64u + lane];
    const unsigned long long live_mask = live[w];
    const bool is_live = ((live_mask >> lane) & 1ull) != 0ull;
    const float prune_scale = prune_scale_v5(L, ro);
    unsigned long long need;
    if (L.unit_mode == RM_UNITS_LATTICE) need = wave_cull_lattice(smem, L.n_grp, x, y, z, thr[64u * w + lane], is_live, live_mask);
    else need = wave_cull_blend(smem, L.n_grp, L.unit_kmax, x, y, z, extra_margin, prune_scale, is_live, live_mask);
    if (lane == 0u) out[w] = need;
}
#endif

}  // namespace rmk
