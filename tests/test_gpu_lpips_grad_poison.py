"""The LPIPS gradient's kernel under LDS poison (the audit of test_gpu_lds_poison.py, for ssg_lpips_layers_backward in
ssg_featmetric.hip): the channel slices' five sums go to slice 0 through LDS, the pixel's six scalars come back to every
slice through the same words, and a workgroup writes them again trip after trip past the grid cap, so a read of a word
that the same trip has not written would see whatever the LDS held.  The profiling build fills the LDS of every CU with
a word in front of every launch; every output must equal the product build's bit for bit (the same sources and
-ffp-contract=off, one writer per element; the profiling switches touch the host side of a launch only).  The outputs
hold NaN by contract (all-zero vectors), so bits are compared, under four words: two NaN patterns, a small-integer
pattern and all ones."""
import pytest
import torch

from test_gpu_lds_poison import PATTERNS, poisoned

WORDS = PATTERNS + [0xFFC00001, 0xFFFFFFFF]


@pytest.mark.gpu
@pytest.mark.parametrize("word", WORDS)
def test_lpips_grad_kernel_under_lds_poison(word):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_gpu_lpips_grad as tg
    want = tg.poison_cases()
    with poisoned(word):
        got = tg.poison_cases()
    assert len(got) == len(want) == 2 * sum(len(c[2]) for c in tg.C.cases(256, 1024))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(tg._bits(a), tg._bits(b)), i
