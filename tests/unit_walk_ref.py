"""The single-unit path of the generated march kernel (csrc/rm_jit.h "Single-unit steps"), as a binary32 NumPy model.  TEST
INFRASTRUCTURE; a plain module without fixtures.

A march step whose unit mask holds ONE unit u returns what the straight-line code returns with every other unit skipped.  The
model folds the postfix program that way, from the command stream and the skipping rules alone (rm_kernel_v5.h "Pruning"): a skipped
leaf is +inf where it is pushed or intersected with, and leaves the accumulator alone where it is fused with a Union or a
Subtraction; operators on sub-trees apply as they stand.  Operators are the device's: v_min_f32 / v_max_f32, where a NaN operand
loses and -0 < +0.  For leaf values that are numbers this is the fold with every other leaf AT +inf (fold_at_inf; min(acc, +inf) and
max(acc, -inf) return acc), which the tests check too; a NaN accumulator is where the two differ, and the skipping form is what
the kernel runs.

The generator's own classification is read from the source it emits (walk_classes): per class the units, the leaf kind and
the expression in the leaf's value."""
import re

import numpy as np

from test_gpu_query import commands

F = np.float32
INF = F(np.inf)
LEAVES = {0: "sphere", 1: "box", 10: "cylinder"}
UNION, SUBTRACTION, INTERSECTION = 100, 101, 102
# leaf values the classification has to be exact for: numbers of both signs, both zeros, both infinities, NaN
PROBES = tuple(F(x) for x in (1.5, -2.0, 0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e38, 1.0e-45))


def hw_min(a, b):
    """v_min_f32 on quiet operands"""
    a, b = F(a), F(b)
    if np.isnan(a):
        return b
    if np.isnan(b):
        return a
    if a == b:
        return a if np.signbit(a) else b
    return a if a < b else b


def hw_max(a, b):
    a, b = F(a), F(b)
    if np.isnan(a):
        return b
    if np.isnan(b):
        return a
    if a == b:
        return b if np.signbit(a) else a
    return a if a > b else b


def vmin(a, b):
    return hw_min(a, b)


def vmax_negb(a, b):
    return hw_max(a, -F(b))


def fmax_(a, b):
    return hw_max(a, b)


def vmin_pinf(b):
    return hw_min(INF, b)


_OPS = {UNION: vmin, SUBTRACTION: vmax_negb, INTERSECTION: fmax_}


def leaf_kinds(cc, words):
    """kind name of every unit (= bounded leaf), in program order"""
    return [LEAVES[op] for _, op, _ in commands(words, cc) if op in LEAVES]


def _fused(cmds, i, depth):
    """the decoder fuses "leaf; operator" into one record when the leaf is the operator's right operand and a value is below it"""
    return i + 1 < len(cmds) and depth >= 1 and cmds[i + 1][1] in _OPS


def fold_one_unit(cc, words, u, x):
    """the program with unit u's leaf = x and every other unit SKIPPED"""
    cmds = commands(words, cc)
    stack, unit, i = [], 0, 0
    while i < len(cmds):
        op = cmds[i][1]
        if op in LEAVES:
            mine = unit == u
            unit += 1
            if _fused(cmds, i, len(stack)):
                mode = cmds[i + 1][1]
                acc = stack.pop()
                if mine:
                    stack.append(_OPS[mode](acc, x))
                else:
                    stack.append(INF if mode == INTERSECTION else acc)
                i += 2
                continue
            stack.append(F(x) if mine else INF)
        else:
            assert op in _OPS, "not a lattice program: opcode %d" % op
            b = stack.pop()
            a = stack.pop()
            stack.append(_OPS[op](a, b))
        i += 1
    assert len(stack) == 1
    return stack[0]


def fold_at_inf(cc, words, u, x):
    """the program with unit u's leaf = x and every other leaf AT +inf, every operator applied"""
    stack, unit = [], 0
    for _, op, _ in commands(words, cc):
        if op in LEAVES:
            stack.append(F(x) if unit == u else INF)
            unit += 1
        else:
            b = stack.pop()
            a = stack.pop()
            stack.append(_OPS[op](a, b))
    return stack[0]


def walk_body(src):
    m = re.search(r"float map_scene_walk\(.*?\) \{\n(.*?)\n\}", src, re.S)
    return None if m is None else [l.strip() for l in m.group(1).splitlines()]


_LEAF_CALL = re.compile(r"spec_(sphere|box|cylinder)<FAST>\(r, qx, qy, qz, tiny\)")


def walk_classes(src):
    """[(mask or None for "every unit left", kind or None, expression in X)] in the order the generated code tests them, or None when
    the source has no single-unit path"""
    body = walk_body(src)
    if body is None:
        return None
    k = next(i for i, l in enumerate(body) if l.startswith("const LdsF r = lp + 8u * (uint32_t)__builtin_ctz(m);"))
    out = []
    for line in body[k + 1:]:
        if line == "}":
            break
        m = re.match(r"(?:if \(\(m & 0x([0-9a-f]+)u\) != 0u\) \{)?\s*(?:n_eval \+= 1u;)?\s*return (.*?);(?: \})?$", line)
        assert m, line
        kind = _LEAF_CALL.search(m.group(2))
        out.append((int(m.group(1), 16) if m.group(1) else None, kind.group(1) if kind else None, _LEAF_CALL.sub("X", m.group(2))))
    return out


def class_of(classes, u):
    for mask, kind, expr in classes:
        if mask is None or (mask >> u) & 1:
            return kind, expr
    return None            # the step takes the straight-line code


def evaluate(expr, x):
    return F(eval(expr, {"__builtins__": {}}, {"X": F(x), "inf": INF, "vmin": vmin, "vmax_negb": vmax_negb, "fmax_": fmax_,
                                               "vmin_pinf": vmin_pinf}))


def same_bits(a, b):
    a, b = F(a), F(b)
    return (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32)
