"""The rule behind the per-tile primitive masks ("Per-tile primitive masks"), pinned without a GPU: the
un-ANDed tile test as tests/tile_mask_ref.py models it in binary64 -- an entry's bit is 0 iff the tile's cone clears the entry's
bounding sphere or, for a box, its centre ray misses the box grown by D rho -- must never drop an entry that a sample ray of the
tile meets.  Random programs of tests/fuzz_programs.py (all three classes), their own cameras on a frame eight times the fuzz
frame's size, every tile of it, the numpy oracle's binary32 sample rays against cull_ref's binary64 zones."""
import numpy as np
import pytest

import fuzz_programs as FP
import tile_mask_ref as TM
from prepass_ref import all_tiles
from test_cull_tables_cpu import decode
from test_gpu_cull_bounds import table_zones

W, H = 8 * FP.W, 8 * FP.H          # 168 x 104: 21 x 13 tiles, the same aspect as the fuzz frame the cameras were chosen on
_TOTALS = {"tiles": 0, "touching": 0, "met": 0, "mask": 0, "entries": 0, "cases": 0}


@pytest.mark.parametrize("cls", FP.CLASSES)
def test_the_model_mask_keeps_every_entry_a_sample_ray_meets(oracle, cls):
    for seed in FP.SEEDS:
        c = FP.case(oracle, cls, seed)
        d = decode(c.cc, c.words)
        if d["cull_veto"] or TM.n_entries(d) == 0:          # (a Plane, or nothing bounded: no tables, no mask)
            continue
        u = oracle.orbit_uniforms((float(W), float(H)), events=c.events)[0]
        ud = FP.uniforms_dict(u)
        ro64 = np.array([ud["inv_view"][12 + k] for k in range(3)], dtype=np.float32).astype(np.float64)
        zones, bits = table_zones(d, ro64, c.limits[0]), TM.entry_bits(d)
        assert len(zones) == len(bits) and max(bits) < TM.n_entries(d)
        txy = all_tiles(W, H)
        ro, mask, met = TM.tile_truth(ud, W, H, txy, zones, bits)
        assert np.all(ro == ro64)
        dropped = met & ~mask
        assert not dropped.any(), "%s: tile %s: a sample ray meets entry bits %#x the model's mask leaves out" % (
            FP.describe(c), txy[np.argmax(dropped != 0)].tolist(), int(dropped[np.argmax(dropped != 0)]))
        _TOTALS["cases"] += 1
        _TOTALS["tiles"] += len(txy)
        _TOTALS["touching"] += int((met != 0).sum())
        _TOTALS["met"] += int(TM.popcount(met).sum())
        _TOTALS["mask"] += int(TM.popcount(mask).sum())
        _TOTALS["entries"] += len(txy) * len(bits)


def test_the_model_mask_is_a_mask(oracle):
    """Not vacuous: over the cases above the model names a small part of all (tile, entry) pairs, and no more than the entries
    really met plus one per touching tile and one per tile that touches nothing (the cone's circumscription of a square tile)."""
    if _TOTALS["cases"] == 0:
        for cls in FP.CLASSES:
            test_the_model_mask_keeps_every_entry_a_sample_ray_meets(oracle, cls)
    print("model masks over %(cases)d cases: %(tiles)d tiles, %(touching)d touching, |E| %(met)d, mask population %(mask)d of %(entries)d" % _TOTALS)
    assert _TOTALS["cases"] >= 12 and _TOTALS["touching"] > 1000
    assert _TOTALS["met"] <= _TOTALS["mask"] <= _TOTALS["met"] + _TOTALS["tiles"]
    assert _TOTALS["mask"] < 0.5 * _TOTALS["entries"]
