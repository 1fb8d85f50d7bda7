"""SPSR's gradient-map kernels under LDS poison (the audit of test_gpu_lds_poison.py, for ssg_spsr.hip): every sums
kernel folds its four waves' fp64 partials through LDS, and the folding workgroup adds the partials through an LDS
tree, so a word read before it is written would be whatever the LDS held.  The profiling build fills the LDS of every CU
with a word in front of every launch; every output must equal the product build's bit for bit (the same sources and
-ffp-contract=off, fixed-order sums; the profiling switches touch the host side of a launch only)."""
import pytest
import torch

from test_gpu_lds_poison import PATTERNS, poisoned


@pytest.mark.gpu
@pytest.mark.parametrize("word", PATTERNS)
def test_spsr_kernels_under_lds_poison(word):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_gpu_spsr as ts
    want = ts.poison_cases()
    with poisoned(word):
        got = ts.poison_cases()
    assert len(got) == len(want) == 69
    for i, (a, b) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(b.double()).all()), i
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(ts._bits(a), ts._bits(b)), i
