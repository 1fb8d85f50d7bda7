"""The LPIPS and DISTS criteria's kernels under LDS poison (the audit of test_gpu_lds_poison.py, for ssg_featmetric.hip):
the LPIPS kernel adds its channel slices through LDS and folds its four waves through LDS once per unit, trip after
trip; the moments kernel folds five sums per chunk; both finishing kernels add through an LDS tree, layer after layer.
A word read before it is written would be whatever the LDS held.  The profiling build fills the LDS of every CU with a
word in front of every launch; every output must equal the product build's bit for bit (the same sources and
-ffp-contract=off, fixed-order sums; the profiling switches touch the host side of a launch only)."""
import pytest
import torch

from test_gpu_lds_poison import PATTERNS, poisoned

# the audit's two words, and two more: all ones (-1 as a count or an index, a NaN as a value) and +infinity
WORDS = PATTERNS + [0xFFFFFFFF, 0x7F800000]


@pytest.mark.gpu
@pytest.mark.parametrize("word", WORDS)
def test_featmetric_kernels_under_lds_poison(word):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_gpu_featmetric as tf
    want = tf.poison_cases()
    with poisoned(word):
        got = tf.poison_cases()
    assert len(got) == len(want) == 6 + 6
    for i, (a, b) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(b).all()), i
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(tf._bits(a), tf._bits(b)), i
