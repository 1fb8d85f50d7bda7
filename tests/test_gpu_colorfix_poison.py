"""The colour-correction kernels under LDS poison (the audit of test_gpu_lds_poison.py, for ssg_colorfix.hip): the tile
pass keeps the haloed difference and five levels of row and column passes in two buffers of 128,016 bytes of dynamic LDS
and forms each level on a region that shrinks with it, so a tap outside the region the previous level wrote would read
whatever the LDS held; the statistics kernels fold their sums through LDS.  The profiling build fills the LDS of every CU
with a word in front of every launch; every output must equal the product build's bit for bit, the NaN plane included
(the same sources and -ffp-contract=off, fixed-order sums; the profiling switches touch the host side of a launch
only)."""
import pytest
import torch

from test_gpu_lds_poison import PATTERNS, poisoned


@pytest.mark.gpu
@pytest.mark.parametrize("word", PATTERNS)
def test_colorfix_kernels_under_lds_poison(word):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_gpu_colorfix as tc
    want = tc.poison_cases()
    with poisoned(word):
        got = tc.poison_cases()
    assert len(got) == len(want) == 15
    for i in range(13):
        assert bool(torch.isfinite(want[i].double()).all()), i
    assert bool(torch.isnan(want[13][:, :, 1]).all()) and bool(torch.isnan(want[14]).all())      # the NaN plane
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(tc._bits(a), tc._bits(b)), i
