"""The spectral-normalisation kernels under LDS poison (the audit of test_gpu_lds_poison.py, for ssg_specnorm.hip): every
fold hands its four wave sums to all threads through LDS, several times per unit and unit after unit, so a word read
before it is written would be whatever the LDS held.  The profiling build fills the LDS of every CU with a word in
front of every launch; every output must equal the product build's bit for bit (the same sources and
-ffp-contract=off, sums in a fixed order)."""
import numpy as np
import pytest
import torch

from test_gpu_lds_poison import PATTERNS, poisoned

# the audit's two words, and two more: all ones (a NaN as a value) and +infinity
WORDS = PATTERNS + [0xFFFFFFFF, 0x7F800000]


def _cases(dev):
    """Every output of a training call, its backward and an eval call on the seventeen-layer set and the tall layer."""
    import specnorm_cases as C
    import test_gpu_specnorm as T
    outputs = []
    for shapes in (C.MIXED_17, C.TALL):
        run = T.Run(dev, C.layer_set(shapes, seed=15))
        grads = C.gradients(shapes)
        for training in (True, False):
            outs, saved = run.forward(training)
            outputs += outs + run.backward(saved, grads) + [saved.cpu().numpy()]
    return outputs


@pytest.mark.gpu
@pytest.mark.parametrize("word", WORDS)
def test_specnorm_kernels_under_lds_poison(word):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    want = _cases(dev)
    with poisoned(word):
        got = _cases(dev)
    assert len(got) == len(want) == 2 * 2 * 17 + 2 + 2 * 2 + 2
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.isfinite(b).all(), i
        assert a.dtype == b.dtype and a.shape == b.shape
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), i
