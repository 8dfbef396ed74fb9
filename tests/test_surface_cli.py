"""python -m ray_marching_amd.surface on the GPU: the JSON report of a small scene without and with
--supports, and the exit status of --fail-on."""
import json
import math

import pytest

from ray_marching_amd import surface

pytestmark = pytest.mark.gpu


def run(capsys, *args):
    status = surface.main(list(args))
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    return status, json.loads(lines[0])


def test_sphere_report(capsys):
    status, r = run(capsys, "--scene", "g1", "--res", "64")
    assert status == 0 and r["failed"] == [] and r["shape"] == [64, 64, 64]
    # R = 12.6 points: within the larger recorded error of the neighbouring radii of section 25's table
    assert abs(r["area"] / (4.0 * math.pi) - 1.0) <= 0.0108
    assert r["facet_area"] == pytest.approx(sum(r["facets"].values()), rel=1e-12) and set(r["facets"]) == {"pos_x", "neg_x", "pos_y", "neg_y", "pos_z", "neg_z"}
    assert r["facets"]["pos_x"] == r["facets"]["neg_x"] > 0.0                      # a closed surface
    assert r["facet_area"] > r["area"]                                          # the staircase overestimates a round surface
    assert r["volume"] == pytest.approx(4.0 * math.pi / 3.0, rel=0.02) and r["volume_area_ratio"] == pytest.approx(r["volume"] / r["area"])
    assert "contact" not in r and r["stats"]["bricks"] > 0


def test_supports_report_and_gates(capsys):
    args = ("--scene", "g8", "--res", "48", "--supports", "--up", "+z", "--r2", "1")
    status, r = run(capsys, *args)
    c = r["support_counts"]
    cell = r["step"][0] * r["step"][1]
    assert status == 0 and r["up"] == "+z" and r["r2"] == 1 and c["overhang"] > 0
    assert r["contact"] == pytest.approx((c["runs"] + c["landings"]) * cell, rel=1e-12)
    assert r["contact_facet_area"] >= r["contact"] and r["contact_area"] > 0.0
    assert r["footprint"] == pytest.approx(c["base"] * cell, rel=1e-12)
    assert r["overhang_skin"] == pytest.approx(c["overhang"] * cell, rel=1e-12)   # every overhang point has nothing of the part below it
    status, r2 = run(capsys, *args, "--fail-on", "area>%g,contact>%g" % (r["area"] * 2.0, r["contact"] * 0.5))
    assert status == 2 and len(r2["failed"]) == 1 and r2["failed"][0].startswith("contact = ")
    status, r3 = run(capsys, "--scene", "g8", "--res", "48", "--fail-on", "area>%g,contact>0" % (r["area"] * 0.5))
    assert status == 2 and len(r3["failed"]) == 1 and r3["failed"][0].startswith("area = ")
    status, _ = run(capsys, "--scene", "g8", "--res", "48", "--fail-on", "area>%g" % (r["area"] * 2.0))
    assert status == 0
