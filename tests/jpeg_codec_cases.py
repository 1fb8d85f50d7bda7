"""The inputs the JPEG round trip is tested on, shared by the CPU tests (restatement against Pillow), the fixture's
generator (tests/golden/make_golden_jpeg_codec.py) and the GPU tests (kernel against restatement and fixture)."""
import io
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f31_jpeg_codec.npz")

# (H, W): a side below, at and above the 8-pixel block and the 16-pixel MCU; even heights with a partial last MCU row
# (24, 72: there the downsampled chroma rows are replicated, not the full-resolution ones); odd sides; W <= 4, where
# libjpeg upsamples with its box filter
SIZES = [(1, 1), (1, 40), (2, 2), (2, 40), (7, 9), (8, 8), (8, 16), (10, 10), (10, 16), (15, 17), (16, 16), (17, 33),
         (24, 16), (24, 24), (31, 47), (37, 53), (40, 40), (72, 72), (33, 100), (64, 65), (100, 34), (24, 40), (72, 100)]
SMALL_SIZES = [(4, 4), (2, 3), (3, 2), (36, 1), (37, 1), (40, 3), (40, 4), (5, 5), (3, 40), (9, 6)]
QUALITIES = [1, 5, 30, 50, 75, 95, 100]
CONTENTS = ["noise", "ramp", "saturated", "constant", "checker1", "checker8"]


def content(kind, H, W, C, seed=0):
    """(H, W) for C = 1, (H, W, 3) for C = 3, uint8"""
    rng = np.random.default_rng([seed, H, W, C])
    shape = (H, W) if C == 1 else (H, W, C)
    yy, xx = np.mgrid[:H, :W]
    if kind == "noise":
        a = rng.integers(0, 256, shape)
    elif kind == "saturated":
        a = rng.integers(0, 2, shape) * 255
    elif kind == "constant":
        a = np.broadcast_to(rng.integers(0, 256, (1, 1) if C == 1 else (1, 1, C)), shape)
    elif kind == "ramp":                        # modular ramps, a different slope per channel
        a = np.stack([(yy * (7 + 4 * c) + xx * (3 + 2 * c)) % 256 for c in range(C)], -1).reshape(shape)
    elif kind in ("checker1", "checker8"):      # +-255 checkerboard, the channels in opposite phase: the range limit
        p = 1 if kind == "checker1" else 8
        b = (((yy // p) + (xx // p)) & 1) * 255
        a = np.stack([b if c != 1 else 255 - b for c in range(C)], -1).reshape(shape)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a, dtype=np.uint8)


def pillow_roundtrip(img, quality):
    """Pillow's save(format='JPEG', quality=q) + open: libjpeg(-turbo) at its defaults, as cv2 calls it"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=int(quality))
    out = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
    assert out.shape == img.shape, (out.shape, img.shape)
    return out


# the fixture: (H, W, C, quality, content).  The GPU tests' shapes first (test_gpu_jpeg_codec.py).
FIXTURE_CASES = [
    (8, 8, 3, 75, "noise"), (16, 16, 3, 30, "noise"), (17, 33, 3, 95, "noise"), (24, 40, 3, 50, "noise"),
    (72, 72, 3, 75, "noise"), (31, 47, 3, 5, "noise"), (64, 65, 3, 90, "noise"), (130, 70, 3, 60, "noise"),
    (65, 65, 3, 85, "ramp"), (8, 16, 1, 75, "noise"), (37, 53, 1, 30, "noise"), (130, 70, 1, 100, "noise"),
    (24, 40, 3, 100, "saturated"), (72, 72, 3, 1, "saturated"), (31, 47, 3, 100, "ramp"), (17, 33, 3, 1, "ramp"),
    (40, 40, 3, 1, "checker1"), (40, 40, 3, 100, "checker1"), (40, 40, 3, 1, "checker8"), (40, 40, 3, 100, "checker8"),
    (24, 24, 1, 1, "checker1"), (24, 24, 1, 100, "checker8"), (16, 16, 3, 75, "constant"), (1, 1, 3, 75, "noise"),
    (2, 3, 3, 75, "noise"), (3, 2, 3, 30, "noise"), (4, 4, 3, 95, "noise"), (36, 1, 3, 75, "noise"),
    (1, 40, 3, 50, "noise"), (40, 4, 3, 75, "saturated"), (40, 5, 3, 75, "saturated"), (5, 3, 1, 30, "noise"),
    (100, 34, 3, 95, "saturated"), (33, 100, 3, 75, "ramp"), (10, 16, 3, 100, "noise"), (15, 17, 3, 50, "saturated"),
]


def fixture_name(case):
    return "%dx%d_c%d_q%d_%s" % case


def load_fixture():
    """{case: (input, Pillow's output)} as recorded"""
    z = np.load(GOLDEN)
    return {c: (z["in_" + fixture_name(c)], z["out_" + fixture_name(c)]) for c in FIXTURE_CASES}
