"""The resize kernel under LDS poison (the audit of test_gpu_lds_poison.py, for ssg_resample.hip): a workgroup keeps its
coefficient rows, the bounds, the input footprint (aligned dwords, of which a row's first and last hold bytes outside the
footprint) and the byte intermediate in up to 160 KiB of dynamic LDS whose layout changes with the call, so a tap outside
what the same workgroup staged would read whatever the LDS held.  The profiling build fills the LDS of every CU with a
word in front of every launch; every output of test_gpu_prep.py's cases must equal the product build's bit for bit."""
import pytest
import torch

from test_gpu_lds_poison import PATTERNS, poisoned


@pytest.mark.gpu
@pytest.mark.parametrize("word", PATTERNS)
def test_resize_kernel_under_lds_poison(word):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_gpu_prep as tp
    want = tp.poison_cases()
    with poisoned(word):
        got = tp.poison_cases()
    assert len(got) == len(want) == len(tp.CASES) + 2
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), i
    # and the product build's outputs are the restatement's (test_gpu_prep.py), here for the first and the last case
    for i in (0, len(tp.CASES) - 1):
        assert torch.equal(want[i].cpu(), torch.from_numpy(tp._pair(tp.CASES[i])[1].copy()))
