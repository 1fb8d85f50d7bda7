"""The GAN criteria's kernels under LDS poison (the audit of test_gpu_lds_poison.py, for ssg_gan.hip): the sums kernel
folds its four waves' fp64 pairs through LDS, and the folding workgroup adds the partial pairs through an LDS tree, so a
word read before it is written would be whatever the LDS held.  The profiling build fills the LDS of every CU with a word
in front of every launch; every output must equal the product build's bit for bit (the same sources and
-ffp-contract=off, fixed-order sums; the profiling switches touch the host side of a launch only)."""
import pytest
import torch

from test_gpu_lds_poison import PATTERNS, poisoned


@pytest.mark.gpu
@pytest.mark.parametrize("word", PATTERNS)
def test_gan_kernels_under_lds_poison(word):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_gpu_gan as tg
    want = tg.poison_cases()
    with poisoned(word):
        got = tg.poison_cases()
    assert len(got) == len(want) == 42
    for i, (a, b) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(b.double()).all()), i
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(tg._bits(a), tg._bits(b)), i
