"""Integer restatement of libjpeg's baseline JPEG round trip (encode at a quality, decode again), in numpy.

What the reference reaches through ``cv2.imencode`` / ``cv2.imdecode`` and what Pillow's ``Image.save(format='JPEG',
quality=q)`` + ``Image.open`` gives: ``jpeg_set_quality(q, force_baseline=TRUE)``, 4:2:0 for colour, the "islow" integer
DCT pair, fancy upsampling, no smoothing.  Entropy coding is lossless, so the decoded pixels are fixed by eight stages,
each a function of its own here so that a failing comparison can name the stage:

    rgb_to_ycc -> downsample -> fdct -> quantise (quant_tables) -> [dequantise] -> idct -> upsample -> ycc_to_rgb

Every shift is arithmetic (numpy's ``>>`` on signed integers floors).  The DCTs take a dtype so that the int32
evaluation the kernel uses can be compared with an int64 one.  This file is the specification
ssl_amd/csrc/ssg_jpegcodec.hip is held to; tests/test_cpu_jpeg_codec.py holds it to Pillow.

The `wrong` argument of roundtrip() switches ONE rule to a plausible wrong one (the sensitivity tests: the case set
must tell each apart):  'bias2' a constant bias of 2 in the downsample; 'fullres_rows' the bottom MCU rows replicated
at full resolution before the downsample; 'box' box instead of fancy upsampling; 'upsample_uncropped' fancy upsampling
of the uncropped chroma planes; 'half_even' round-half-to-even in the quantiser; 'wrap' the portable C library's 10-bit
wrap of the inverse DCT's output where libjpeg-turbo's SIMD code saturates.
"""
import numpy as np

CONST_BITS, PASS1_BITS = 13, 2
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172

# the standard tables of the JPEG specification (Annex K), in natural (row, column) order
LUMA_BASE = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64).reshape(8, 8)
CHROMA_BASE = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99], np.int64).reshape(8, 8)


def quant_tables(quality):
    """(luminance, chrominance) 8 x 8 int64 tables of jpeg_set_quality(quality, force_baseline)."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality must be 1 .. 100, got {quality!r}")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (LUMA_BASE, CHROMA_BASE))


def rgb_to_ycc(rgb):
    """(H, W, 3) uint8 -> Y, Cb, Cr int64 planes (16-bit fixed point)."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(plane, rows, cols):
    """replicates the last row / column out to (rows, cols)"""
    return np.pad(plane, ((0, rows - plane.shape[0]), (0, cols - plane.shape[1])), mode="edge")


def downsample(plane, const_bias=False):
    """2 x 2 mean of a plane of even sides, bias 1, 2, 1, 2 ... along the output columns."""
    s = plane[0::2, 0::2] + plane[0::2, 1::2] + plane[1::2, 0::2] + plane[1::2, 1::2]
    bias = np.full(s.shape[1], 2, np.int64) if const_bias else 1 + (np.arange(s.shape[1]) & 1)
    return (s + bias[None, :]) >> 2


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first, dtype):
    """the forward transform along the LAST axis of (..., 8)"""
    d = d.astype(dtype)
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) * (1 << PASS1_BITS), (t10 - t11) * (1 << PASS1_BITS)
    else:
        out[0], out[4] = _descale(t10 + t11, PASS1_BITS), _descale(t10 - t11, PASS1_BITS)
    z1 = (t12 + t13) * F_0_541
    out[2] = _descale(z1 + t13 * F_0_765, n)
    out[6] = _descale(z1 - t12 * F_1_847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    out[7] = _descale(t4 + z1 + z3, n)
    out[5] = _descale(t5 + z2 + z4, n)
    out[3] = _descale(t6 + z2 + z3, n)
    out[1] = _descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def fdct(blocks, dtype=np.int64):
    """(..., 8, 8) samples 0 .. 255 -> coefficients carrying a factor 8 (rows first, then columns)."""
    x = _fdct_1d(np.asarray(blocks).astype(dtype) - 128, True, dtype)
    return np.swapaxes(_fdct_1d(np.swapaxes(x, -1, -2), False, dtype), -1, -2)


def quantise(coef, table, half_even=False):
    """sign(c) ((|c| + 4 Q) // (8 Q)): half away from zero on the x 8 scaled coefficient."""
    c = np.asarray(coef).astype(np.int64)
    if half_even:
        return np.rint(c / (8.0 * table)).astype(np.int64)
    return np.sign(c) * ((np.abs(c) + 4 * table) // (8 * table))


def _idct_1d(d, first, dtype):
    """the inverse transform along the LAST axis of (..., 8)"""
    d = d.astype(dtype)
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * F_0_541
    t2, t3 = z1 - z3 * F_1_847, z1 + z2 * F_0_765
    t0, t1 = (d[..., 0] + d[..., 4]) * (1 << CONST_BITS), (d[..., 0] - d[..., 4]) * (1 << CONST_BITS)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175
    t0, t1, t2, t3 = t0 * F_0_298, t1 * F_2_053, t2 * F_3_072, t3 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS + 3
    out = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([_descale(o, n) for o in out], axis=-1)


def idct(coef, dtype=np.int64, wrap=False):
    """(..., 8, 8) dequantised coefficients -> samples 0 .. 255 (columns first, then rows, + 128, range limit)."""
    x = np.swapaxes(_idct_1d(np.swapaxes(np.asarray(coef), -1, -2), True, dtype), -1, -2)
    x = _idct_1d(x, False, dtype).astype(np.int64)
    if wrap:                                    # the portable code's table, indexed through a 10-bit mask
        x = ((x + 512) & 1023) - 512
    return np.clip(x + 128, 0, 255)


def _blocks(plane):
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2)


def _unblocks(blocks):
    nby, nbx = blocks.shape[:2]
    return blocks.swapaxes(1, 2).reshape(nby * 8, nbx * 8)


def code_plane(plane, table, dtype=np.int64, half_even=False, wrap=False):
    """a plane whose sides are multiples of 8 through fdct, quantise, dequantise and idct"""
    q = quantise(fdct(_blocks(plane), dtype), table, half_even)
    return _unblocks(idct(q * table, dtype, wrap))


def upsample(c, box=False):
    """h2v2 upsampling of a (h, w) chroma plane to (2 h, 2 w).  Fancy (triangle) for w > 2, else (and for `box`)
    replication: libjpeg picks its box upsampler for a downsampled width of 1 or 2."""
    c = np.asarray(c).astype(np.int64)
    h, w = c.shape
    if box or w <= 2:
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    above, below = np.vstack([c[:1], c[:-1]]), np.vstack([c[1:], c[-1:]])
    v = np.empty((2 * h, w), np.int64)
    v[0::2], v[1::2] = 3 * c + above, 3 * c + below
    out = np.empty((2 * h, 2 * w), np.int64)
    out[:, 2::2] = (3 * v[:, 1:] + v[:, :-1] + 8) >> 4
    out[:, 1:-1:2] = (3 * v[:, :-1] + v[:, 1:] + 7) >> 4
    out[:, 0] = (4 * v[:, 0] + 8) >> 4
    out[:, -1] = (4 * v[:, -1] + 7) >> 4
    return out


def ycc_to_rgb(y, cb, cr):
    """int planes -> (H, W, 3) uint8"""
    y, cb, cr = (np.asarray(p).astype(np.int64) for p in (y, cb - 128, cr - 128))
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def encode_planes(img, wrong=None):
    """The planes as the encoder's transforms see them: [Y] for (H, W), [Y, Cb, Cr] for (H, W, 3); Y padded to whole
    MCUs (8 x 8 for grey, 16 x 16 for colour), the chroma planes downsampled and padded to whole blocks."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    if img.ndim == 2:
        return [_pad(img.astype(np.int64), -(-H // 8) * 8, -(-W // 8) * 8)]
    Hm, Wm = -(-H // 16) * 16, -(-W // 16) * 16
    y, cb, cr = rgb_to_ycc(img)
    planes = [_pad(y, Hm, Wm)]
    for c in (cb, cr):
        if wrong == "fullres_rows":
            planes.append(downsample(_pad(c, Hm, Wm)))
        else:       # one replicated row at most, down to an even height; the DOWNSAMPLED rows fill the MCU row
            planes.append(_pad(downsample(_pad(c, H + (H & 1), Wm), wrong == "bias2"), Hm // 2, Wm // 2))
    return planes


def roundtrip(img_u8, quality, dtype=np.int64, wrong=None):
    """uint8 (H, W) or (H, W, 3) -> the same shape after libjpeg's baseline encode at `quality` and decode."""
    img = np.asarray(img_u8)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3) or 0 in img.shape:
        raise ValueError(f"roundtrip takes uint8 (H, W) or (H, W, 3), got {img.dtype} {img.shape}")
    H, W = img.shape[:2]
    tables = quant_tables(quality)
    kw = dict(dtype=dtype, half_even=wrong == "half_even", wrap=wrong == "wrap")
    planes = encode_planes(img, wrong)
    y = code_plane(planes[0], tables[0], **kw)[:H, :W]
    if img.ndim == 2:
        return y.astype(np.uint8)
    hc, wc = -(-H // 2), -(-W // 2)
    chroma = []
    for p in planes[1:]:
        c = code_plane(p, tables[1], **kw)
        if wrong != "upsample_uncropped":
            c = c[:hc, :wc]                     # cropped BEFORE upsampling: the last real row / column is the context
        chroma.append(upsample(c, wrong == "box")[:H, :W])
    return ycc_to_rgb(y, chroma[0], chroma[1])
