"""Write coverage of a draw ("Write coverage"): every pixel of the region written, nothing outside it.

TEST INFRASTRUCTURE.  A draw into device memory gets a buffer whose every byte is a sentinel: the region the draw owns, with
guard_rows rows of the frame's width in front of it and behind it.  check() then looks at raw bits:

  * no pixel of the region still carries the sentinel -- a pixel the draw did not write.  The oracle's alpha is always 1.0
    (255 in the 8-bit formats), so an alpha that is still the sentinel is never a legitimate pixel;
  * the region equals the reference bit for bit (two NaNs count as equal, as in test_gpu_parity.assert_same);
  * every guard byte is still the sentinel -- a store outside the region (a ragged tile, a band's first row, another frame of
    a batch, a 16-byte pixel where 4 bytes were asked for) lands there.

A failure names the first offending pixel as (frame, row, col) of the region and its 8 x 8 tile (col // 8, row // 8) -- rows
count from the region's first row, which is how the kernels cut a band into tiles --, and says so when the whole tile is
unwritten: a dropped tile reads as one.

Pixels are (..., 4) float32 (16 bytes) or (..., 4) uint8 (4 bytes); a buffer is (guard_rows + frames * rows + guard_rows, W, 4),
a reference (rows, W, 4) or (frames, rows, W, 4).  check() takes numpy arrays and torch tensors alike, so that
tests/test_write_coverage_cpu.py can hand it corrupted arrays without a GPU."""
import numpy as np

F32_SENTINEL = 0x7FC5A5A5       # a quiet NaN with a payload no arithmetic produces, in all four channels
U8_SENTINEL = 0xA5              # neither 0 nor 255


def _np_dtype(dtype):
    name = str(dtype).split(".")[-1]        # numpy dtypes, numpy scalar types and torch dtypes alike
    if "float32" in name:
        return np.dtype(np.float32)
    if "uint8" in name:
        return np.dtype(np.uint8)
    raise ValueError("pixels are float32 or uint8, not %r" % (dtype,))


def _shape3(shape):
    """(frames, rows, W) of a (rows, W, 4) or (frames, rows, W, 4) shape."""
    shape = tuple(int(x) for x in shape)
    if len(shape) == 3:
        shape = (1,) + shape
    if len(shape) != 4 or shape[3] != 4:
        raise ValueError("a frame is (rows, W, 4) or (frames, rows, W, 4), not %r" % (shape,))
    return shape[:3]


def sentinel_array(shape, dtype):
    """A host array of `shape` ((..., 4)) with every byte of every pixel the sentinel."""
    dt = _np_dtype(dtype)
    if dt == np.uint8:
        return np.full(shape, U8_SENTINEL, dtype=np.uint8)
    return np.full(shape, F32_SENTINEL, dtype=np.uint32).view(np.float32)


def guarded_host(shape, dtype, guard_rows):
    """guarded() in host memory."""
    frames, rows, W = _shape3(shape)
    return sentinel_array((2 * int(guard_rows) + frames * rows, W, 4), dtype)


def guarded(shape, dtype, guard_rows, device="cuda:0"):
    """A torch device buffer (guard_rows + frames * rows + guard_rows, W, 4) of `dtype` (float32 or uint8, numpy's or torch's),
    every byte the sentinel.  region_ptr() is where the draw writes."""
    import torch
    frames, rows, W = _shape3(shape)
    n = (2 * int(guard_rows) + frames * rows, W, 4)
    if _np_dtype(dtype) == np.uint8:
        buf = torch.full(n, U8_SENTINEL, dtype=torch.uint8, device=device)
    else:
        buf = torch.full(n, F32_SENTINEL, dtype=torch.int32, device=device).view(torch.float32)
    torch.cuda.synchronize(device)
    return buf


def region_ptr(buf, guard_rows):
    """Device address of the region's first pixel."""
    return buf.data_ptr() + int(guard_rows) * buf.shape[1] * 4 * buf.element_size()


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.ascontiguousarray(a)


def _words(a):
    """(n, W) uint32, one word per 8-bit pixel; (n, W, 4) uint32 for float pixels."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint8:
        return a.view(np.uint32)[..., 0]
    if a.dtype == np.float32:
        return a.view(np.uint32)
    raise ValueError("pixels are float32 or uint8, not %r" % (a.dtype,))


def written(a):
    """(n, W) bool: the pixels of a host array whose alpha is no longer the sentinel."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint8:
        return a[..., 3] != U8_SENTINEL
    return a.view(np.uint32)[..., 3] != F32_SENTINEL


def untouched(a):
    """(n, W) bool: the pixels of a host array whose every byte is still the sentinel."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint8:
        return np.all(a == U8_SENTINEL, axis=-1)
    return np.all(a.view(np.uint32) == F32_SENTINEL, axis=-1)


def _first(mask):
    """(frame, row, col) of the first set entry of a (frames, rows, W) mask, in memory order."""
    return tuple(int(x) for x in np.argwhere(mask)[0])


def _where(f, r, c):
    return "(frame %d, row %d, col %d), tile (%d, %d)" % (f, r, c, c // 8, r // 8)


def check(buf, ref, what=""):
    """buf: a guarded buffer after the draw; ref: the reference frame(s).  The guard is what buf has more than ref, half in
    front and half behind.  Raises AssertionError naming the first offending pixel."""
    buf, ref = _host(buf), np.ascontiguousarray(ref)
    frames, rows, W = _shape3(ref.shape)
    assert buf.dtype == ref.dtype, "%s: buffer is %s, reference %s" % (what, buf.dtype, ref.dtype)
    assert buf.ndim == 3 and buf.shape[1:] == (W, 4), "%s: buffer %r does not hold rows of %d pixels" % (what, buf.shape, W)
    extra = buf.shape[0] - frames * rows
    assert extra >= 0 and extra % 2 == 0, "%s: buffer of %d rows around %d x %d rows" % (what, buf.shape[0], frames, rows)
    g = extra // 2
    pre = ("%s: " % what) if what else ""
    region = buf[g:g + frames * rows].reshape(frames, rows, W, 4)
    want = ref.reshape(frames, rows, W, 4)
    # 1. nothing of the sentinel is left in the region
    missing = ~written(region)
    if missing.any():
        f, r, c = _first(missing)
        ty, tx = r // 8, c // 8
        tile = missing[f, ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]
        n = int(missing.sum())
        if tile.all() and tile.size > 1:
            raise AssertionError("%swhole tile (%d, %d) of frame %d was not written: its %d pixels from (frame %d, row %d, col %d) on "
                                 "still hold the sentinel (%d unwritten pixels in all)" % (pre, tx, ty, f, tile.size, f, r, c, n))
        raise AssertionError("%spixel %s was not written: it still holds the sentinel (%d unwritten pixels in all, %d of them in "
                             "this tile)" % (pre, _where(f, r, c), n, int(tile.sum())))
    # 2. the region is the reference, bit for bit
    a, b = _words(region.reshape(frames * rows, W, 4)), _words(want.reshape(frames * rows, W, 4))
    differ = a != b
    if ref.dtype == np.float32:
        differ &= ~(np.isnan(region.reshape(frames * rows, W, 4)) & np.isnan(want.reshape(frames * rows, W, 4)))
        differ = differ.any(axis=-1)
    differ = differ.reshape(frames, rows, W)
    if differ.any():
        f, r, c = _first(differ)
        raise AssertionError("%spixel %s holds %s, the reference %s (%d of %d pixels differ)" % (
            pre, _where(f, r, c), region[f, r, c].tolist(), want[f, r, c].tolist(), int(differ.sum()), differ.size))
    # 3. nothing was written outside the region
    for name, part in (("leading", buf[:g]), ("trailing", buf[g + frames * rows:])):
        hit = ~untouched(part)
        if hit.any():
            r, c = (int(x) for x in np.argwhere(hit)[0])
            dist = g - r if name == "leading" else r + 1
            raise AssertionError("%sthe %s guard was written: guard row %d, col %d (%d row%s %s the region) holds %s; %d guard pixels "
                                 "in all" % (pre, name, r, c, dist, "" if dist == 1 else "s",
                                             "before" if name == "leading" else "after the last row of", part[r, c].tolist(),
                                             int(hit.sum())))
