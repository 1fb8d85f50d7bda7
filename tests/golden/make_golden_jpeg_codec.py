"""Record f31_jpeg_codec.npz: small images and what Pillow's JPEG round trip makes of them.

    python tests/golden/make_golden_jpeg_codec.py

Needs Pillow with JPEG support (libjpeg or libjpeg-turbo), which calls `jpeg_set_quality(q, force_baseline)` and keeps
the library's defaults -- 4:2:0 for colour, the integer "islow" DCT, fancy upsampling -- as OpenCV's imencode /
imdecode do.  For every case of tests/jpeg_codec_cases.py:FIXTURE_CASES the file holds `in_<name>` (the uint8 image,
(H,W) or (H,W,3)) and `out_<name>` (`Image.open` of `Image.save(format='JPEG', quality=q)`), and `pillow` /
`libjpeg` name the versions that wrote it.  On a machine whose Pillow is built differently the fixture still pins the
bytes that tests/jpeg_codec_reference.py, and through it the kernel, must produce.  Only data is stored."""
import os
import sys
sys.dont_write_bytecode = True

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_codec_cases as K  # noqa: E402

LIMIT = 1 << 20          # the most a committed file may take


def main():
    import PIL
    from PIL import features
    arrays = {"pillow": np.array(PIL.__version__),
              "libjpeg": np.array("%s%s" % (features.version("jpg"),
                                            " (turbo)" if features.check_feature("libjpeg_turbo") else ""))}
    for case in K.FIXTURE_CASES:
        H, W, C, q, kind = case
        a = K.content(kind, H, W, C, seed=31)
        arrays["in_" + K.fixture_name(case)] = a
        arrays["out_" + K.fixture_name(case)] = K.pillow_roundtrip(a, q)
    np.savez_compressed(K.GOLDEN, **arrays)
    size = os.path.getsize(K.GOLDEN)
    print(f"{K.GOLDEN}: {len(K.FIXTURE_CASES)} cases, {size} bytes")
    if size > LIMIT:
        raise SystemExit(f"{size} bytes is over the {LIMIT} a committed file may take: drop or shrink cases")


if __name__ == "__main__":
    main()
