"""The NIQE kernels under LDS poison (the audit of test_gpu_lds_poison.py, for ssg_niqe.hip): niqe_plane2 stages its
inputs and the row pass in LDS, niqe_features the haloed tile, the MSCN block and its 30 fixed-order sums (117,720 bytes
of dynamic LDS), niqe_fit its partial means, Sigma and the Cholesky factor.  The profiling build fills the LDS of every
CU with a word in front of every launch; every output must equal the product build's bit for bit, NaN entries included
(the same sources and flags, fixed-order sums; the profiling switches touch the host side of a launch only)."""
import pytest
import torch

from test_gpu_lds_poison import PATTERNS, poisoned


@pytest.mark.gpu
@pytest.mark.parametrize("word", PATTERNS)
def test_niqe_kernels_under_lds_poison(word):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_gpu_niqe as tn
    want = tn.poison_cases()
    with poisoned(word):
        got = tn.poison_cases()
    assert len(got) == len(want) == 12
    assert bool(torch.isfinite(want[0]).all()) and bool(torch.isfinite(want[4]).all())
    assert bool(torch.isnan(want[9]).any()) and bool(torch.isfinite(want[8]).all())    # the NaN row; its batch's scores
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(tn._bits(a), tn._bits(b)), i
