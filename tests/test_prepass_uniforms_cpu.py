"""The uniform blocks the pre-pass's tile verdicts are tested under (tests/prepass_ref.py: variants) are not a vacuous list: by the
numpy reference alone -- camera_rays for all sixteen samples of every pixel, the oracle's floor codes -- enough of them have many
tiles that are truly all sky and many that truly lie in one checker cell, several with a horizon that is not horizontal, so that
tests/test_gpu_prepass_uniforms.py can demand settled tiles of them.  No device is needed."""
import numpy as np
import pytest

import prepass_ref as P

W, H = P.BASE_SIZE


@pytest.fixture(scope="module")
def truth(oracle):
    """{variant: (number of truly-sky tiles, number of truly-one-cell tiles, codes of those, rows of horizon tilt)}"""
    out = {}
    for name, u in P.variants(oracle, W, H).items():
        ud = P.udict(u)
        sky, cell = P.tile_truth(ud, W, H)
        out[name] = (int(sky.sum()), int((cell >= 0).sum()), set(np.unique(cell[cell >= 0]).tolist()), P.horizon_tilt_rows(ud, W, H))
    return out


def rich_variants(truth):
    return [n for n, (n_sky, n_cell, _, _) in truth.items() if n_sky >= 20 and n_cell >= 20]


def test_the_frame_sizes_end_the_last_workgroup_where_they_should():
    for (w, h), rest in ((P.BASE_SIZE, 1), (P.SIZE_31, 31)):
        assert w % 8 == 0 and h % 8 == 0 and (w // 8) * (h // 8) % 32 == rest
    assert P.RAGGED_SIZE[0] % 8 != 0 and P.RAGGED_SIZE[1] % 8 != 0
    assert ((P.RAGGED_SIZE[0] + 7) // 8, (P.RAGGED_SIZE[1] + 7) // 8) == (P.BASE_SIZE[0] // 8, P.BASE_SIZE[1] // 8)


def test_enough_variants_have_sky_tiles_and_one_cell_tiles(truth):
    for name, t in truth.items():
        print("%-20s truly sky %4d, truly one cell %4d (bits %s), horizon tilt %3d rows" % (name, t[0], t[1], sorted(t[2]), t[3]))
    assert set(truth) == set(P.VARIANT_NAMES) and (W // 8) * (H // 8) == 1025
    rich = rich_variants(truth)
    assert len(rich) >= 6, rich
    # a horizon that is not horizontal: the share of sky differs by more than a tile's height between the frame's two sides
    tilted = [n for n in rich if truth[n][3] > 8]
    assert len(tilted) >= 3, tilted
    assert {"roll30", "roll90"} <= set(tilted)
    assert any(truth[n][2] == {0, 1} for n in tilted)


def test_the_reference_counts_of_the_issue_stand(truth):
    """Figures of the numpy reference at 328 x 200 (1025 tiles), recorded when the variants were chosen."""
    want = {"still": (820, 27), "roll30": (801, 72), "roll90": (700, 183), "off_axis": (574, 217), "just_above_floor": (820, 164),
            "extent_small": (779, 3), "on_floor": (1025, 0)}
    assert {n: truth[n][:2] for n in want} == want


def test_cameras_that_see_no_floor_cell(truth):
    assert truth["on_floor"][1] == 0 and truth["nan_rays"][1] == 0
    assert truth["on_floor"][0] == 1025 and truth["nan_rays"][0] == 1025      # fd > 0 fails for fd = 0 and for NaN: every miss is black


def test_look_down_shows_one_cell_tiles_and_tiles_across_cell_edges(oracle, truth):
    n_sky, n_cell, bits, _ = truth["look_down"]
    assert n_cell >= 100 and bits == {0, 1}
    assert 1025 - n_sky - n_cell >= 100          # tiles on the horizon or across a cell edge
    ud = P.udict(P.variants(oracle, W, H)["look_down"])
    sky, cell = P.tile_truth(ud, W, H)
    floor_rows = ~sky.reshape(H // 8, W // 8).any(axis=1)                     # tile rows without a sky tile: below the horizon
    mixed = (cell.reshape(H // 8, W // 8) < 0) & floor_rows[:, None]
    assert mixed.sum() >= 50                     # all floor, yet more than one cell


def test_corner_samples_do_not_bound_a_tile_under_noisy_rolls(oracle):
    """What the sky rule's slack is for, by the reference alone: under noisy_rolls there are tiles whose four extreme samples all
    point up although a sample between them reaches the floor; under the plain roll there are none."""
    blocks = P.variants(oracle, W, H)
    n_bad = {}
    for name in ("roll30", "noisy_rolls"):
        ud = P.udict(blocks[name])
        sky, _ = P.tile_truth(ud, W, H)
        n_bad[name] = int((P.corner_samples_point_up(ud, W, H) & ~sky).sum())
    assert n_bad["roll30"] == 0 and n_bad["noisy_rolls"] >= 1, n_bad
