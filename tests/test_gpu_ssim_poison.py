"""The SSIM criterion's kernels under LDS poison (the audit of test_gpu_lds_poison.py, for ssg_ssim.hip): the tile pass
keeps the haloed images, five moments, the three partials on the ring and their row pass in 151,160 bytes of dynamic LDS,
the second row pass over the buffer the moments were in, and walks several tiles per workgroup past the grid cap, so a
tap outside what the same tile pass wrote would read whatever the LDS held; both kernels fold their sums through LDS.
The profiling build fills the LDS of every CU with a word in front of every launch; every output must equal the product
build's bit for bit (the same sources and -ffp-contract=off, fixed-order sums; the profiling switches touch the host
side of a launch only)."""
import pytest
import torch

from test_gpu_lds_poison import PATTERNS, poisoned


@pytest.mark.gpu
@pytest.mark.parametrize("word", PATTERNS)
def test_ssim_kernels_under_lds_poison(word):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_gpu_ssim as ts
    want = ts.poison_cases()
    with poisoned(word):
        got = ts.poison_cases()
    assert len(got) == len(want) == 16
    for i, (a, b) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(b.double()).all()), i
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(ts._bits(a), ts._bits(b)), i
