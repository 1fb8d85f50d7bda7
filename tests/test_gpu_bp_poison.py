"""The back-projection kernels under LDS poison (the audit of test_gpu_lds_poison.py, for ssg_bp.hip): bp_fwd stages
the input tile with its mirrored halo and the row pass's output in LDS, bp_bwd the upstream values, the column
gather's output and the taps, and both keep their block sums there.  The profiling build fills the LDS of every CU
with a word in front of every launch; every output must equal the product build's bit for bit (the same sources and
flags, fixed-order sums; the profiling switches touch the host side of a launch only)."""
import pytest
import torch

from test_gpu_lds_poison import PATTERNS, poisoned


@pytest.mark.gpu
@pytest.mark.parametrize("word", PATTERNS)
def test_bp_kernels_under_lds_poison(word):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_gpu_bp as tb
    want = tb.poison_cases()
    with poisoned(word):
        got = tb.poison_cases()
    assert len(got) == len(want) == 24
    for i, (a, b) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(b.float()).all()), i
        assert torch.equal(a, b), (i, float((a.float() - b.float()).abs().max()))
