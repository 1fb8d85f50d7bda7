"""The ragged degradation kernels under LDS poison (the audit of test_gpu_lds_poison.py, for ssg_blindsr.hip): the
convolution folds every tile's window and halo, and the flipped taps, into LDS before it reads them, so a word read
before it is written would be whatever the LDS held.  The profiling build fills the LDS of every CU with a word in front
of every launch; every output must equal the product build's bit for bit (the same sources and -ffp-contract=off, one
writer per element; the profiling switches touch the host side of a launch only)."""
import pytest
import torch

from test_gpu_lds_poison import PATTERNS, poisoned


@pytest.mark.gpu
@pytest.mark.parametrize("word", PATTERNS)
def test_blindsr_kernels_under_lds_poison(word):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_gpu_blindsr as tb
    want = tb.poison_cases()
    with poisoned(word):
        got = tb.poison_cases()
    assert len(got) == len(want) == 2 * 49 + 27 + 13
    for i, (a, b) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(b.double()).all()), i
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(tb._bits(a), tb._bits(b)), i
