"""The device sort on the GPU (csrc/rm_sort.h through rm_selftest_sort): the pairs == numpy's stable argsort of the keys' low `bits`
bits, for sizes around a wave, a workgroup pass and the tile, for more than 1024 workgroups, for every number of passes and short
last digits; stability on equal keys; key bits above `bits` do not take part; two runs are identical."""
import ctypes as C

import numpy as np
import pytest

from ray_marching_amd import _ffi, renderer

pytestmark = pytest.mark.gpu

TILE = _ffi.SORT_TILE
SIZES = (1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1)
BITS = (1, 8, 9, 16, 40, 64)
MANY = 1025 * TILE + 77              # 1026 tiles: more than 1024 workgroups, and a table scan of more than one block per digit row


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    yield r
    r.close()


def sort(res, keys, values, bits):
    keys, values = np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(values, dtype=np.uint32)
    ok, ov = np.empty_like(keys), np.empty_like(values)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _ffi.check(res._h, _ffi.hip_lib().rm_selftest_sort(res._h, p(keys), p(values), len(keys), bits, p(ok), p(ov)))
    return ok, ov


def mask(bits):
    return np.uint64((1 << bits) - 1)


def expect(keys, values, bits):
    order = np.argsort(keys & mask(bits), kind="stable")
    return keys[order], values[order]


def random_keys(rng, n, bits):
    """Keys of 64 random bits, many of them equal in their low `bits` bits (a few distinct low parts), so that ties occur."""
    k = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    few = rng.integers(0, 1 << 63, 7, dtype=np.uint64)
    tie = rng.random(n) < 0.5
    low = np.where(tie, few[rng.integers(0, 7, n)], k) & mask(bits)
    return (k & ~mask(bits)) | low


@pytest.mark.parametrize("bits", BITS)
def test_sizes_and_bits(res, bits):
    rng = np.random.default_rng(100 + bits)
    for n in SIZES:
        keys, values = random_keys(rng, n, bits), rng.integers(0, 1 << 32, n, dtype=np.uint32)
        gk, gv = sort(res, keys, values, bits)
        wk, wv = expect(keys, values, bits)
        assert np.array_equal(gk, wk) and np.array_equal(gv, wv), (n, bits)


@pytest.fixture(scope="module")
def many():
    rng = np.random.default_rng(7)
    return random_keys(rng, MANY, 20), np.arange(MANY, dtype=np.uint32)


def test_more_than_1024_workgroups(res, many):
    keys, values = many
    gk, gv = sort(res, keys, values, 20)
    wk, wv = expect(keys, values, 20)
    assert np.array_equal(gk, wk) and np.array_equal(gv, wv)


def test_two_runs_are_identical(res, many):
    keys, values = many
    a, b = sort(res, keys, values, 20), sort(res, keys, values, 20)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("n", (65, TILE + 1, 5 * TILE + 3))
def test_equal_keys_keep_their_order(res, n):
    values = np.arange(n, dtype=np.uint32)
    for bits in (1, 9, 64):
        gk, gv = sort(res, np.full(n, 0x0123456789ABCDEF, dtype=np.uint64), values, bits)
        assert np.array_equal(gv, values) and np.all(gk == np.uint64(0x0123456789ABCDEF))


@pytest.mark.parametrize("bits", (1, 8, 9, 16, 40))
def test_bits_above_do_not_take_part(res, bits):
    """Keys that differ only above `bits` must not move -- also where the last digit is short (9: one bit of the second digit)."""
    rng = np.random.default_rng(bits)
    n = 3 * TILE + 5
    keys = (rng.integers(0, 1 << 62, n, dtype=np.uint64) << np.uint64(bits)) | np.uint64(1 if bits > 1 else 0)
    values = np.arange(n, dtype=np.uint32)
    gk, gv = sort(res, keys, values, bits)
    assert np.array_equal(gv, values) and np.array_equal(gk, keys)


def test_arguments(res):
    L = _ffi.hip_lib()
    k, v = np.zeros(4, np.uint64), np.zeros(4, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.rm_selftest_sort(res._h, p(k), p(v), 0, 8, p(k), p(v)) == _ffi.RM_ERR_ARG
    assert L.rm_selftest_sort(res._h, p(k), p(v), 4, 0, p(k), p(v)) == _ffi.RM_ERR_ARG
    assert L.rm_selftest_sort(res._h, p(k), p(v), 4, 65, p(k), p(v)) == _ffi.RM_ERR_ARG
    assert L.rm_selftest_sort(res._h, None, p(v), 4, 8, p(k), p(v)) == _ffi.RM_ERR_NULL
