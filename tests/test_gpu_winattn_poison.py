"""The window-attention kernels under LDS poison (the audit of test_gpu_lds_poison.py, for ssg_winattn.hip): a unit keeps
its q, k, v and dout tiles, the head's bias column, the tokens' source pixels and labels and P / dS in LDS, reuses the
tiles for its outputs and takes unit after unit, so a word read before it is written would be whatever the LDS held.
The profiling build fills the LDS of every CU with a word in front of every launch; every output must equal the product
build's bit for bit (the same sources and -ffp-contract=off, sums in a fixed order)."""
import numpy as np
import pytest
import torch

from test_gpu_lds_poison import PATTERNS, poisoned

# the audit's two words, and two more: all ones (a NaN as a value) and +infinity
WORDS = PATTERNS + [0xFFFFFFFF, 0x7F800000]


def _cases(dev):
    """out, dqkv and dtable of the 16 x 24 case (all nine labels, head_dim 30 padded to 32) and the batch case."""
    import test_gpu_winattn as T
    import winattn_cases as C
    outputs = []
    for name in ("labels_s4", "batch_d10"):
        outputs += T.run(dev, C.by_name(name))
    return outputs


@pytest.mark.gpu
@pytest.mark.parametrize("word", WORDS)
def test_winattn_kernels_under_lds_poison(word):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    want = _cases(dev)
    with poisoned(word):
        got = _cases(dev)
    assert len(got) == len(want) == 6
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.isfinite(b).all(), i
        assert a.dtype == b.dtype and a.shape == b.shape
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), i
