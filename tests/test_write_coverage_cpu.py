"""write_coverage.check on hand-corrupted host arrays: the proof that the GPU tests of tests/test_gpu_write_coverage.py can
fail, and that a failure names the right place.  No GPU."""
import re

import numpy as np
import pytest

import write_coverage as WC

W, H, G = 19, 21, 3     # ragged in both directions: tiles (2, *) and (*, 2) hang over the frame


def frame(dtype, frames=1, seed=5):
    """A plausible reference: random colours, alpha 1.0 / 255."""
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.uint8:
        ref = rng.integers(0, 256, (frames, H, W, 4), dtype=np.uint8)
        ref[..., 3] = 255
    else:
        ref = rng.random((frames, H, W, 4), dtype=np.float32)
        ref[..., 3] = 1.0
    return ref


def drawn(ref):
    """The guarded buffer a correct draw of `ref` leaves."""
    buf = WC.guarded_host(ref.shape, ref.dtype, G)
    buf[G:G + ref.shape[0] * H] = ref.reshape(-1, W, 4)
    return buf


def sentinel_pixel(dtype):
    return WC.sentinel_array((4,), dtype)


def fails(buf, ref, *fragments):
    with pytest.raises(AssertionError) as e:
        WC.check(buf, ref, "case")
    msg = str(e.value)
    for frag in fragments:
        assert re.search(frag, msg), (frag, msg)
    return msg


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_a_correct_draw_passes(dtype):
    for frames in (1, 3):
        ref = frame(dtype, frames)
        WC.check(drawn(ref), ref)
        WC.check(drawn(ref), ref[0] if frames == 1 else ref)     # (rows, W, 4) and (frames, rows, W, 4) alike
    nan = frame(np.float32)
    nan[0, 4, 5, 0] = np.float32(np.nan)
    other = nan.copy()
    other.view(np.uint32)[0, 4, 5, 0] = 0xFFC00001                 # another NaN: equal, as in assert_same
    WC.check(drawn(nan), other)


def test_sentinels_are_what_the_contract_excludes():
    f = WC.sentinel_array((2, 2, 4), np.float32)
    assert np.isnan(f).all() and (f.view(np.uint32) == WC.F32_SENTINEL).all()
    assert (WC.F32_SENTINEL >> 22) & 0x1FF == 0x1FF               # exponent all ones and the quiet bit
    b = WC.sentinel_array((2, 2, 4), np.uint8)
    assert (b == WC.U8_SENTINEL).all() and WC.U8_SENTINEL not in (0, 255)
    assert not WC.written(f).any() and WC.untouched(f).all() and not WC.written(b).any() and WC.untouched(b).all()
    g = WC.guarded_host((3, H, W, 4), np.uint8, G)
    assert g.shape == (2 * G + 3 * H, W, 4) and g.dtype == np.uint8 and WC.untouched(g).all()


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["float", "8bit"])
def test_one_unwritten_pixel(dtype):
    ref = frame(dtype, 2)
    buf = drawn(ref)
    buf[G + H + 13, 17] = sentinel_pixel(dtype)                    # frame 1, row 13, col 17
    fails(buf, ref, r"pixel \(frame 1, row 13, col 17\), tile \(2, 1\) was not written", r"1 unwritten pixels in all")


def test_one_unwritten_tile():
    ref = frame(np.float32)
    buf = drawn(ref)
    buf[G + 8:G + 16, 8:16] = sentinel_pixel(np.float32)
    fails(buf, ref, r"whole tile \(1, 1\) of frame 0 was not written", r"its 64 pixels from \(frame 0, row 8, col 8\)", r"64 unwritten")
    # a ragged tile at the frame's corner: 3 x 5 pixels of it exist
    buf = drawn(ref)
    buf[G + 16:G + H, 16:W] = sentinel_pixel(np.float32)
    fails(buf, ref, r"whole tile \(2, 2\) of frame 0 was not written", r"its 15 pixels")
    # most of a tile is not a tile
    buf = drawn(ref)
    buf[G + 8:G + 16, 8:16] = sentinel_pixel(np.float32)
    buf[G + 8, 8] = ref[0, 8, 8]
    fails(buf, ref, r"pixel \(frame 0, row 8, col 9\), tile \(1, 1\) was not written", r"63 unwritten pixels in all, 63 of them in this tile")


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["float", "8bit"])
def test_one_pixel_in_the_leading_guard(dtype):
    ref = frame(dtype)
    buf = drawn(ref)
    buf[G - 1, 4] = ref[0, 0, 4]                                    # the row right in front of the region
    fails(buf, ref, r"the leading guard was written: guard row 2, col 4 \(1 row before the region\)", r"1 guard pixels")
    buf = drawn(ref)
    buf[0, 0, 1] = 7 if np.dtype(dtype) == np.uint8 else 0.5       # one channel of the very first pixel
    fails(buf, ref, r"the leading guard was written: guard row 0, col 0 \(3 rows before the region\)")


def test_one_pixel_in_the_trailing_guard():
    ref = frame(np.float32, 2)
    buf = drawn(ref)
    buf[G + 2 * H, 18] = ref[1, 0, 18]                              # the row right behind frame 1
    fails(buf, ref, r"the trailing guard was written: guard row 0, col 18 \(1 row after the last row of the region\)")
    buf = drawn(ref)
    buf[-1, -1] = ref[0, 0, 0]
    fails(buf, ref, r"the trailing guard was written: guard row 2, col 18 \(3 rows after")


def test_a_16_byte_pixel_in_a_4_byte_frame_reaches_the_trailing_guard():
    """What a float store into an 8-bit frame does: pixel i lands at byte 16 i, four pixels wide."""
    ref = frame(np.uint8)
    buf = WC.guarded_host(ref.shape, np.uint8, 3 * H + G)          # as the GPU tests size it: room for all of it
    flat = buf.reshape(-1)
    at = (3 * H + G) * W * 4
    flat[at:at + H * W * 4] = ref.reshape(-1)
    i = H * W // 4 + 5                                              # a pixel whose 16-byte slot lies behind the region
    flat[at + 16 * i:at + 16 * i + 16] = np.frombuffer(np.array([0.25, 0.5, 0.75, 1.0], np.float32).tobytes(), np.uint8)
    fails(buf, ref, r"the trailing guard was written")


def test_a_wrong_value_in_a_written_region():
    ref = frame(np.float32)
    buf = drawn(ref)
    buf.view(np.uint32)[G + 20, 3, 2] ^= 1                         # one ulp in one channel
    fails(buf, ref, r"pixel \(frame 0, row 20, col 3\), tile \(0, 2\) holds", r"1 of 399 pixels differ")
    ref8 = frame(np.uint8)
    buf = drawn(ref8)
    buf[G + 1, 9, 0] ^= 1
    fails(buf, ref8, r"pixel \(frame 0, row 1, col 9\), tile \(1, 0\) holds")
    # the right frame at the wrong place: frame 1 of a batch written where frame 0 belongs
    two = frame(np.float32, 2)
    buf = drawn(two)
    buf[G:G + H] = two[1]
    fails(buf, two, r"pixel \(frame 0, row 0, col 0\), tile \(0, 0\) holds")


def test_shapes_that_do_not_fit_are_refused():
    ref = frame(np.float32)
    with pytest.raises(AssertionError):
        WC.check(drawn(ref)[1:], ref)                               # an odd number of guard rows
    with pytest.raises(AssertionError):
        WC.check(drawn(ref), frame(np.uint8))
    with pytest.raises(AssertionError):
        WC.check(drawn(ref)[:, :W - 1], ref)
