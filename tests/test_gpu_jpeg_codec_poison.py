"""The JPEG round-trip kernels under LDS poison (the audit of test_gpu_lds_poison.py, for ssg_jpegcodec.hip): a workgroup
keeps up to 48 blocks of 8 x 8 samples in LDS, of which those that lie outside the image -- Y blocks past the right and
bottom edge of a ragged tile, chroma blocks of the halo beyond the image's block grid -- are never written, so a
transform or an upsampling tap that reached one would read whatever the LDS held; the quantiser's tables and the
256-entry float table are filled by the workgroup itself.  The profiling build fills the LDS of every CU with a word
in front of every launch; every output of test_gpu_jpeg_codec.py's cases must equal the product build's bit for bit."""
import numpy as np
import pytest
import torch

from test_gpu_lds_poison import PATTERNS, poisoned


@pytest.mark.gpu
@pytest.mark.parametrize("word", PATTERNS)
def test_jpeg_codec_kernels_under_lds_poison(word):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import jpeg_codec_cases as K
    import test_gpu_jpeg_codec as tj
    want = tj.poison_cases()
    with poisoned(word):
        got = tj.poison_cases()
    assert len(got) == len(want) == len(K.FIXTURE_CASES) + 3
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), i
    # and the product build's outputs are the restatement's (test_gpu_jpeg_codec.py), here for the first and last case
    for i in (0, len(K.FIXTURE_CASES) - 1):
        assert np.array_equal(want[i].cpu().numpy(), tj._want(K.FIXTURE_CASES[i])[1])
