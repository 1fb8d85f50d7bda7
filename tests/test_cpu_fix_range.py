"""Conditions on the INPUTS of tests/test_gpu_fix_range.py, shown on the fp64 oracle alone (no GPU): the step-edge input
reaches the limit of the deterministic gradient's fixed-point conversion when one wave sums all offset rows of a dense
tile, and stays well below it at the split every small test gets; the restated device rules (scale, wave slots, offset-row
split) hold at their edges; and the oracle refuses image sizes its reflect fold cannot index."""
import math

import numpy as np
import pytest

import fix_range_reference as fr
from oracle import ssg_oracle as orc


@pytest.fixture(scope="module")
def control():
    """The 32 x 96 step-edge block alone under a dense mask at (49,13), sigma 1, weights 1e3: 24 dense tiles of 4 x 32."""
    sr, gt = fr.control_pair(fr.CASE_SEED)
    ref = fr.loss_reference(sr, gt, np.ones((32, 96), np.float32), 49, 13, 1.0, 1e3, 1e3, want_grad=False)
    return sr, ref


def test_step_edge_reaches_the_conversion_limit_at_one_wave_per_tile(control):
    """reach_bits = log2(max |tile partial| / |G|max) + 35, the lower end of log2 |v * scale| at an exact bound of |G|:
    measured 51.53 with all 49 offset rows in one sum (parts = 1, the split of plans with more tiles than wave slots) --
    past the 2^51 the magic-number conversion holds -- and 49.80 with the rows split five ways (every (49,13) oracle test
    at small size: at most 204 tiles).  The test at one wave per tile can reach the limit, the small ones cannot."""
    sr, ref = control
    one = fr.reach_bits(fr.tile_reach(sr, ref["gD"], ref["pos"], 49, 13, 4, 32, 1))
    five = fr.reach_bits(fr.tile_reach(sr, ref["gD"], ref["pos"], 49, 13, 4, 32, 5))
    print(f"FIXRANGE reference 32x96 (49,13): reach_bits parts=1 {one:.3f}, parts=5 {five:.3f}")
    assert one >= 51.45
    assert five <= one - 1.5


def test_embedded_block_reaches_the_limit_in_the_upper_part_of_the_binade():
    """The same block inside the 132 x 512 image of the GPU test (528 tiles on 256 CUs, parts = 1).  The 32-row image
    above folds most of a tile's region back onto itself (reflect pad 24 + 6 on 32 rows), and distance_backward adds the
    folds into one value; an interior tile has no folds -- and the kernel converts a fold's rows one by one anyway -- so
    the figure that describes a single conversion is this one: measured 50.54, i.e. 2^50.54 .. 2^51.54 by where |G|max
    falls in its binade.  Weights spread over one octave in quarter steps put at least one case at 2^51.29 or more:
    asserted here on the four weights of the GPU test, from the reference's own |G|max."""
    sr, gt, mask, _, tiles = fr.embedded_case(49, 256, fr.CASE_SEED)
    assert tiles == 528 and fr.offset_parts(tiles, 256, 49) == 1
    ref = fr.loss_reference(sr, gt, mask, 49, 13, 1.0, 1e3, 1e3, want_grad=False)
    reach = fr.tile_reach(sr, ref["gD"], ref["pos"], 49, 13, 4, 32, 1)
    gmax = np.abs(ref["gD"]).max()
    conv = [math.log2(gmax * 2 ** (j / 4) * fr.fix_scale(gmax * 2 ** (j / 4)) * reach) for j in range(4)]
    print(f"FIXRANGE reference 132x512 (49,13): reach_bits parts=1 {fr.reach_bits(reach):.3f}, converted log2 {np.round(conv, 2)}")
    assert fr.reach_bits(reach) >= 50.45
    assert max(conv) >= 51.2 and min(conv) >= 50.45


def test_tile_reach_of_one_row_is_the_rows_own_gradient():
    """tile_reach's neighbourhood crop: for a single edge pixel per tile -- at a corner, where the reflect folds land
    inside the crop, and in the interior -- the partial is that row's distance_backward on the whole image."""
    rng = np.random.default_rng(3)
    img = rng.random((3, 40, 70))
    pos = np.array([[0, 1], [21, 40], [39, 69]], np.int32)
    gD = rng.standard_normal((3, 11, 11))
    want = max(np.abs(orc.distance_backward(img, pos[i:i + 1], 11, 5, gD[i:i + 1])).max() for i in range(3))
    got = fr.tile_reach(img, gD, pos, 11, 5, 8, 32, 1) * np.abs(gD).max()
    assert abs(got - want) <= 1e-12 * want
    # offset rows one by one: the parts add up to the whole (linearity), so the sum of their maxima bounds its maximum
    parts = fr.tile_reach(img, gD, pos, 11, 5, 8, 32, 11) * np.abs(gD).max()
    assert 11 * parts >= want


def test_fix_scale_matches_the_bit_formula():
    """grad_fix_scale_of: bound < 2^(e-126) with the biased exponent e clamped at 40 -> scale 2^(35 - (e - 127)): on the
    powers of two, their float32 neighbours on both sides, and the clamp."""
    f32 = np.float32
    for k in range(-90, 31):
        p = f32(math.ldexp(1.0, k))
        up, down = np.nextafter(p, f32(np.inf)), np.nextafter(p, f32(0))
        e = max(k + 127, 40)
        assert fr.fix_scale(p) == math.ldexp(1.0, 35 - (e - 127)) == fr.fix_scale(up)
        assert fr.fix_scale(down) == math.ldexp(1.0, 35 - (max(k - 1 + 127, 40) - 127))
        if k + 127 >= 40:   # the largest |G| of an exact bound lands in [2^35, 2^36)
            assert 2.0 ** 35 <= float(p) * fr.fix_scale(p) < 2.0 ** 36 and float(down) * fr.fix_scale(down) < 2.0 ** 36
    # clamp: every bound below 2^-87 (biased exponent < 40), zero and denormals included, takes the scale of 2^-87
    for b in (0.0, 1e-45, 1e-38, math.ldexp(1.0, -100), float(np.nextafter(f32(math.ldexp(1.0, -87)), f32(0)))):
        assert fr.fix_scale(f32(b)) == math.ldexp(1.0, 35 + 87)
    assert fr.fix_scale(f32(math.ldexp(1.0, -86))) == math.ldexp(1.0, 35 + 86)


def test_offset_parts_follow_the_wave_slots():
    """256 CUs at (49,13): 1,024 wave slots, one wave per tile -> 5, 2, 1 parts at 204, 512, 513 tiles; (25,9): 2,048
    slots, two waves per tile; and the clamp at both ends."""
    assert fr.wave_slots(256, 49) == 1024 and fr.wave_slots(256, 25) == 2048
    assert [fr.offset_parts(n, 256, 49) for n in (204, 512, 513)] == [5, 2, 1]
    assert [fr.offset_parts(n, 256, 49) for n in (1, 205, 256, 257, 341, 342, 1024, 1025, 100000)] == [5, 4, 4, 3, 3, 2, 1, 1, 1]
    assert [fr.offset_parts(n, 256, 25) for n in (204, 205, 512, 513, 1025)] == [5, 4, 2, 1, 1]
    assert fr.tiles_for_one_part(256, 49) == 513 and fr.tiles_for_one_part(256, 25) == 513
    assert fr.tiles_for_one_part(304, 49) == 609 and fr.offset_parts(0, 256, 49) == 5


def test_embedded_case_layout():
    """The large cases: more dense tiles than the device splits, the block on the tile grid at least 30 pixels from every
    border, every other tile exactly one edge pixel."""
    for ks, need, shape in ((49, None, (132, 512)), (25, 1025, (264, 1024))):
        sr, gt, mask, (y0, x0, h, w), tiles = fr.embedded_case(ks, 256, fr.CASE_SEED, need)
        TY = fr.tile_rows(ks)
        assert sr.shape == gt.shape == (3,) + shape and mask.shape == shape and (h, w) == (32, 96)
        assert tiles == (shape[0] // TY) * (shape[1] // 32) and fr.offset_parts(tiles, 256, ks) == 1
        assert min(y0, x0, shape[0] - y0 - h, shape[1] - x0 - w) >= 30
        per_tile = mask.reshape(shape[0] // TY, TY, shape[1] // 32, 32).sum((1, 3))
        inside = np.zeros_like(per_tile, bool)
        inside[y0 // TY:(y0 + h) // TY, x0 // 32:(x0 + w) // 32] = True
        assert (per_tile[inside] == TY * 32).all() and (per_tile[~inside] == 1).all()
        bsr, bgt = fr.control_pair(fr.CASE_SEED)
        assert np.array_equal(sr[:, y0:y0 + h, x0:x0 + w], bsr) and np.array_equal(gt[:, y0:y0 + h, x0:x0 + w], bgt)


@pytest.mark.parametrize("ks,kw,H,W", [(49, 13, 16, 96), (49, 13, 96, 24), (25, 9, 12, 40), (11, 5, 5, 30)])
def test_oracle_refuses_images_not_larger_than_the_reflect_pad(ks, kw, H, W):
    """orc.distance / orc.distance_backward fold indices with one mirror step, valid while the pad k_s // 2 is smaller
    than the side (16 x 96 at (49,13) used to end in a segmentation fault): ValueError, like torch's reflect pad -- and
    the smallest legal side still computes."""
    img = np.random.default_rng(0).random((3, H, W))
    pos = np.array([[0, 0], [H - 1, W - 1]], np.int32)
    with pytest.raises(ValueError):
        orc.distance(img, pos, ks, kw)
    with pytest.raises(ValueError):
        orc.distance_backward(img, pos, ks, kw, np.ones((2, ks, ks)))
    with pytest.raises(ValueError):
        orc.ssg_loss(img[None], img[None], np.ones((1, H, W)), ks, kw, 1.0)
    side = ks // 2 + 1
    ok = np.random.default_rng(1).random((3, side, side))
    pos = np.array([[0, 0], [side - 1, side - 1]], np.int32)
    D = orc.distance(ok, pos, ks, kw)
    assert np.isfinite(D).all() and np.isfinite(orc.distance_backward(ok, pos, ks, kw, np.ones((2, ks, ks)))).all()
