"""The NIQE kernels under LDS poison (the audit of test_gpu_lds_poison.py) past the fixture's six blocks: niqe_fit with
flags counted by two waves and the row lanes on their second trip (`waves`, 70 rows), with NaN rows of five patterns
(`patterns`) and with two good rows (`two_good`).  Scores, features and both planes must equal the product build's bit
for bit, NaN entries included."""
import pytest
import torch

from test_gpu_lds_poison import PATTERNS, poisoned


@pytest.mark.gpu
@pytest.mark.parametrize("word", PATTERNS)
def test_niqe_block_cases_under_lds_poison(word):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_gpu_niqe_blocks as tb
    want = tb.poison_cases()
    with poisoned(word):
        got = tb.poison_cases()
    assert len(got) == len(want) == 4 * len(tb.POISON_CASES)
    for k in range(len(tb.POISON_CASES)):
        assert bool(torch.isfinite(want[4 * k]).all())                 # every one of the three has a score
        assert bool(torch.isnan(want[4 * k + 1]).any())                # and rows with a NaN
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(tb._bits(a), tb._bits(b)), i
