"""The degradation chain's blur, sinc and pulse kernels without a GPU: kernel_reference.py (this project's fp64
statement of ssg_synth_kernels) against the reference's own results, ssl_amd.datapath.draw_kernels against the
reference dataset's seeded runs (fixture F23, tests/golden/make_golden_kernels.py), and the status codes
ssg_synth_kernels decides before it launches anything.

Bound (kernel_reference.within, derived there): |out - ref| <= 2^-23 |ref| + 1e-30, + 1e-12 instead for a sinc kernel;
every element of every case, no mismatch budget."""
import ctypes

import numpy as np
import pytest

import kernel_reference as R
from kernel_reference import KIND_NAMES, RUN_TAGS, explicit_cases, run_records


def test_fixture_covers_what_it_should(golden):
    g = golden("f23_blur_kernels")
    p = g["a_params"]
    kinds, K, P = p[:, 0].astype(int), p[:, 1].astype(int), p[:, 2].astype(int)
    for kind in range(5):
        have = {(k, q) for k, q in zip(K[kinds == kind], P[kinds == kind])}
        assert {(3, 9), (9, 9), (7, 9), (3, 21), (9, 21), (19, 21), (21, 21)} <= have, KIND_NAMES[kind]
    blur = kinds >= 2
    assert {0.1, 5.0} <= set(p[blur, 3]) and {0.1, 5.0} <= set(p[blur, 4])
    assert ((p[:, 3] == p[:, 4]) & (p[:, 5] != 0) & blur).any()
    assert {np.pi, -np.pi} <= set(p[blur, 5])
    for kind in (3, 4):
        assert {0.1, 1.0, 8.0} <= set(p[kinds == kind, 6])
    sinc = p[kinds == 1]
    assert ((sinc[:, 1] == 3) & (sinc[:, 7] == np.pi)).any() and ((sinc[:, 1] == 21) & (sinc[:, 7] == np.pi / 5)).any()
    # sigma 0.1: the tails have underflowed to exact zeros inside the K x K block
    i = int(np.flatnonzero((kinds == 2) & (K == 21) & (p[:, 3] == 0.1) & (p[:, 4] == 0.1))[0])
    assert g[f"a_ref_{i}"][0, 0] == 0 and g[f"a_ref_{i}"][10, 10] == 1
    for tag in RUN_TAGS:
        pad = int(g[f"b_{tag}_pad"])
        assert g[f"b_{tag}_kernels"].shape == (16, 3, pad, pad) and g[f"b_{tag}_kernels"].dtype == np.float32
        assert float(g[f"b_{tag}_cpu_seconds"]) > 0


def test_reference_restatement_reproduces_the_explicit_cases(golden):
    cases = explicit_cases(golden("f23_blur_kernels"))
    assert len(cases) >= 100
    for rec, pad, ref in cases:
        out = R.kernel(rec, pad)
        assert out.shape == ref.shape
        assert R.within(out.astype(np.float32), ref, rec.kind).all(), (rec, pad, R.excess(out.astype(np.float32), ref, rec.kind))


@pytest.mark.parametrize("tag", RUN_TAGS)
def test_draw_kernels_follows_the_dataset_draw_by_draw(golden, tag):
    """Under the fixture's seeds draw_kernels + kernel_reference give the dataset's kernels, and python's and numpy's
    generators end where the reference run left them (their next draws are the recorded ones)."""
    g = golden("f23_blur_kernels")
    recs, pad, next_py, next_np = run_records(g, tag)
    ref = g[f"b_{tag}_kernels"]
    kinds = set()
    for i, sample in enumerate(recs):
        assert len(sample) == 3
        for j, rec in enumerate(sample):
            out = R.kernel(rec, pad).astype(np.float32)
            assert R.within(out, ref[i, j], rec.kind).all(), (tag, i, j, rec, R.excess(out, ref[i, j], rec.kind))
            kinds.add(rec.kind)
    assert next_py == float(g[f"b_{tag}_next_random"]) and next_np == float(g[f"b_{tag}_next_numpy"])
    if tag != "shipped":
        assert kinds == set(KIND_NAMES)
    if tag == "wide":       # both cutoff ranges of the sinc draw: K < 13 and K >= 13
        ks = [r.size for s in recs for r in s[:2] if r.kind == "sinc"]
        assert min(ks) < 13 <= max(ks), ks


def test_draw_kernels_refuses_what_the_dataset_cannot_pad():
    from ssl_amd import datapath
    opt = dict(blur_kernel_size_min=1, blur_kernel_size_max=5, kernel_list=['iso'], kernel_prob=[1], sinc_prob=0,
               blur_sigma=[0.2, 1], betag_range=[0.5, 4], betap_range=[1, 2], blur_kernel_size_min2=1,
               blur_kernel_size_max2=2, kernel_list2=['skew'], kernel_prob2=[1], sinc_prob2=0, blur_sigma2=[0.2, 1],
               betag_range2=[0.5, 4], betap_range2=[1, 2], final_sinc_prob=0)
    with pytest.raises(ValueError, match="padded size 9"):
        datapath.draw_kernels(opt)                       # 11 x 11 into 9 x 9 (np.pad raises in the reference)
    with pytest.raises(NotImplementedError, match="skew"):
        datapath.draw_kernels(opt, pad_to=11)            # the reference has no code for 'skew' either
    with pytest.raises(NotImplementedError):
        datapath.random_mixed_kernels(['iso'], [1], 9, noise_range=[0.75, 1.25])
    with pytest.raises(NotImplementedError):
        datapath.bivariate_Gaussian(9, 1.0, 1.0, 0.0, grid=np.zeros((9, 9, 2)))
    with pytest.raises(ValueError, match="unknown kernel kind"):
        datapath.pack_records([datapath.KernelRecord("skew", 9)])
    with pytest.raises(RuntimeError, match="GPU"):
        datapath.synth_kernels([datapath.KernelRecord("pulse", 1)], 9, device="cpu")


def test_synth_kernels_status_codes_need_no_gpu():
    """What ssg_synth_kernels refuses, it refuses before the copy and the launch: SSG_E_BADARG (-1) for an even size, a
    size above pad_to, pad_to even or above 21, an unknown kind, n < 0 and a null pointer; n == 0 succeeds."""
    from ssl_amd import _lib, datapath
    L = _lib.lib()
    one = ctypes.c_void_p(8)          # never dereferenced: the checks come first
    Rec = datapath.KernelRecord

    def call(records, pad, n=None, host=True, dev=one, out=one):
        arr = datapath.pack_records(records)
        return L.ssg_synth_kernels(arr.ctypes.data if host else None, len(arr) if n is None else n, pad, dev, out, None)

    good = Rec("gaussian", 9, 1.0, 1.0)
    assert call([good, Rec("sinc", 8, omega_c=1.0)], 9) == -1                 # K even
    assert call([good, Rec("gaussian", 11, 1.0, 1.0)], 9) == -1               # K > pad_to
    assert call([good], 10) == -1 and call([good], 23) == -1                  # pad_to even, pad_to > 21
    assert call([Rec("pulse", 1)], 0) == -1 and call([Rec("pulse", 1)], -3) == -1
    bad = datapath.pack_records([good, good])
    for kind in (5, -1):                                                      # an unknown kind
        bad["kind"][1] = kind
        assert L.ssg_synth_kernels(bad.ctypes.data, 2, 9, one, one, None) == -1
    assert call([good], 9, n=-1) == -1
    assert call([good], 9, host=False) == -1 and call([good], 9, dev=None) == -1 and call([good], 9, out=None) == -1
    assert call([], 9) == 0 and call([good], 9, n=0, host=False, dev=None, out=None) == 0
    assert call([], 10) == -1                                                 # (pad_to is checked even for n == 0)
    assert bad.dtype.itemsize == 48 and bad.dtype.fields["sig_x"][1] == 8 and bad.dtype.fields["omega_c"][1] == 40
