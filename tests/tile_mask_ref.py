"""The per-tile primitive mask ("Per-tile primitive masks"), in numpy alone -- nothing here needs a device.
TEST INFRASTRUCTURE, written from the geometry; it shares no code with the kernels.

The pre-pass tests a tile's cone against every entry of the miss-test tables and, instead of ANDing the verdicts, keeps one bit
per entry: set iff the cone does not provably clear the entry.  A ray or a pixel of the tile then tests the set bits only, which
is sound iff NO sample ray of the tile meets the zone of an entry whose bit is 0.  Here are

  entry_bits     which bit of the mask each zone of test_gpu_cull_bounds.table_zones owns (spheres first, then boxes, by slot)
  tile_cones     a cone around every sample direction of a tile, from the numpy oracle's binary32 rays
  touch_mask     the un-ANDed tile test as real-number geometry in binary64: bit k iff neither the entry's bounding sphere nor,
                 for a box, the box inflated by D rho is cleared by the cone
  entries_met    E(tile): the entries some sample ray of the tile really meets (cull_ref's zones, binary64)

tests/test_tile_masks_cpu.py holds touch_mask to that soundness property on random programs; tests/test_gpu_tile_masks.py holds
the device's mask to it and to E."""
import numpy as np

import cull_ref as R
from prepass_ref import tile_samples

F = np.float32
ALL = 0xFFFFFFFF


def entry_bits(d):
    """Bit of the mask for every zone of table_zones(d, ..), in its order: cone entry `slot` for a sphere (for every bounded
    primitive of a program with transforms), n_cone + slot for a box or cylinder."""
    bits = []
    for r in d["rec"]:
        if r["kind"] not in (1, 2, 3) or r["nocull"]:
            continue
        bits.append(r["slot"] if (d["has_xforms"] or r["kind"] == 1) else d["n_sphere"] + r["slot"])
    assert len(set(bits)) == len(bits)
    return bits


def n_entries(d):
    return int(d["n_sphere"]) + int(d["n_box"])


def tile_cones(e, owner, n):
    """(c (n, 3), rho (n,)) binary64: unit centre direction and radius of a cone that holds every sample direction e[i] of tile
    owner[i], |e^ - c| <= rho, with the relative 0.1 % + 2e-6 the device's cone carries for roundings."""
    e64 = e.astype(np.float64)
    e64 = e64 / np.linalg.norm(e64, axis=1, keepdims=True)
    c = np.zeros((n, 3))
    np.add.at(c, owner, e64)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    rho = np.zeros(n)
    np.maximum.at(rho, owner, np.linalg.norm(e64 - c[owner], axis=1))
    return c, rho * 1.001 + 2.0e-6


def touch_mask(zones, bits, ro64, c, rho):
    """The mask of every tile (uint64 array) for cones (c, rho) from ro64.  An entry is cleared iff every direction within rho of c
    clears its bounding sphere, m.c + |m| rho < sqrt(|m|^2 - R^2), or -- a box -- the centre ray misses the box grown by D rho on
    every side, D = |m| + R bounding how far along any of the cone's rays a point of the box can lie."""
    mask = np.zeros(len(c), dtype=np.uint64)
    for z, bit in zip(zones, bits):
        m = np.asarray(z[1], dtype=np.float64) - ro64
        mm = float(np.linalg.norm(m))
        radius = float(z[2]) if z[0] == "ball" else float(np.linalg.norm(z[2]))
        cleared = np.zeros(len(c), dtype=bool)
        if mm > radius:
            cleared = c @ m + mm * rho < np.sqrt(mm * mm - radius * radius)
        if z[0] == "box":
            infl = (mm + radius) * rho
            for i in np.flatnonzero(~cleared):           # (the zone's size differs per tile)
                cleared[i] = not R.meets_box(z[1], np.asarray(z[2]) + infl[i], ro64, c[i][None, :])[0]
        mask |= np.where(cleared, np.uint64(0), np.uint64(1) << np.uint64(bit))
    return mask


def entries_met(zones, bits, ro64, e, owner, n):
    """E(tile) as a mask (uint64 array): bit of every entry whose zone some sample ray of the tile meets."""
    mask = np.zeros(n, dtype=np.uint64)
    e64 = e.astype(np.float64)
    for z, bit in zip(zones, bits):
        hit = np.zeros(n, dtype=bool)
        np.logical_or.at(hit, owner, R.meets_zone(z, ro64, e64))
        mask |= np.where(hit, np.uint64(1) << np.uint64(bit), np.uint64(0))
    return mask


def popcount(m):
    m = np.asarray(m, dtype=np.uint64)
    return np.array([bin(int(x)).count("1") for x in m], dtype=np.int64)


def tile_truth(ud, W, H, txy, zones, bits):
    """(ro64, model mask, E) for tiles txy of a W x H frame under uniforms ud."""
    ro, e, owner = tile_samples(ud, W, H, np.asarray(txy))
    ro64 = ro.astype(np.float64)
    c, rho = tile_cones(e, owner, len(txy))
    return ro64, touch_mask(zones, bits, ro64, c, rho), entries_met(zones, bits, ro64, e, owner, len(txy))
