"""The imresize kernel under LDS poison (the audit of test_gpu_lds_poison.py, for ssg_imresize.hip): a workgroup keeps its
weight rows, the first indices, the mirrored footprint and the fp64 intermediate in up to 160 KiB of dynamic LDS whose
layout changes with the scale, so a tap outside what the same workgroup staged would read whatever the LDS held.  The
profiling build fills the LDS of every CU with a word in front of every launch; every output of test_gpu_imresize.py's
float and byte cases must equal the product build's bit for bit."""
import numpy as np
import pytest
import torch

from test_gpu_lds_poison import PATTERNS, poisoned


@pytest.mark.gpu
@pytest.mark.parametrize("word", PATTERNS)
def test_imresize_kernel_under_lds_poison(word):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_gpu_imresize as ti
    want = ti.poison_cases()
    with poisoned(word):
        got = ti.poison_cases()
    assert len(got) == len(want) == 9 + len(ti.byte_cases()) + 1
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert bool(torch.isfinite(b.float()).all()), i
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), i
    # and the product build's outputs are the restatement's (test_gpu_imresize.py), here for the byte cases
    for (_, s, expect), b in zip(ti.byte_cases(), want[9:]):
        assert np.array_equal(b.cpu().numpy(), expect), s
