"""The degradation chain's blur, sinc and pulse kernels on the MI355X (ssl_amd/csrc/ssg_kernels.hip through
ssl_amd.datapath.synth_kernels) against the reference's own results (fixture F23) and, beyond the fixture, against
kernel_reference.py, which test_cpu_kernels.py pins to the same fixture.

Bound (kernel_reference.within, derived there): |out - ref| <= 2^-23 |ref| + 1e-30, + 1e-12 instead for a sinc kernel,
`ref` an fp32 value; every element of every case, no mismatch budget."""
import functools
import random

import numpy as np
import pytest
import torch

import kernel_reference as R
from kernel_reference import KIND_NAMES, RUN_TAGS, explicit_cases, run_records

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def check(out, ref, records, what):
    """every kernel of `out` (n, P, P) within its kind's bound of `ref`"""
    out = out.cpu().numpy()
    assert out.shape == ref.shape and out.dtype == np.float32
    worst = 0.0
    for i, rec in enumerate(records):
        worst = max(worst, R.excess(out[i], ref[i], rec.kind))
        assert R.within(out[i], ref[i], rec.kind).all(), (what, i, rec, R.excess(out[i], ref[i], rec.kind))
    print(f"KSYN {what}: {len(records)} kernels, {int((out != ref).sum())} of {out.size} elements differ from the "
          f"reference's float, worst |d| / bound = {worst:.3g}")


def test_explicit_cases_vs_reference(golden):
    from ssl_amd import datapath
    cases = explicit_cases(golden("f23_blur_kernels"))
    for pad in (9, 21):
        sel = [c for c in cases if c[1] == pad]
        assert len(sel) >= 40
        out = datapath.synth_kernels([c[0] for c in sel], pad, DEV)          # one launch per padded size
        check(out, np.stack([c[2] for c in sel]), [c[0] for c in sel], f"explicit cases, pad_to {pad}")


@pytest.mark.parametrize("tag", RUN_TAGS)
def test_seeded_runs_vs_reference(golden, tag):
    from ssl_amd import datapath
    g = golden("f23_blur_kernels")
    recs, pad, _, _ = run_records(g, tag)
    flat = [r for sample in recs for r in sample]
    out = datapath.synth_kernels(flat, pad, DEV)
    check(out, g[f"b_{tag}_kernels"].reshape(-1, pad, pad), flat, f"seeded run {tag}")


def test_per_kernel_functions():
    """The reference's function names and arguments, each at one case, against kernel_reference."""
    from ssl_amd import datapath as D
    Rec = D.KernelRecord
    cases = [
        (D.circular_lowpass_kernel(1.9, 7, device=DEV), Rec("sinc", 7, omega_c=1.9), 7),
        (D.circular_lowpass_kernel(2.5, 5, pad_to=9, device=DEV), Rec("sinc", 5, omega_c=2.5), 9),
        (D.circular_lowpass_kernel(2.5, 9, pad_to=False, device=DEV), Rec("sinc", 9, omega_c=2.5), 9),
        (D.bivariate_Gaussian(9, 1.4, 3.0, 0.7, device=DEV), Rec("gaussian", 9, 1.4, 1.4, 0.0), 9),           # isotropic
        (D.bivariate_Gaussian(9, 1.4, 3.0, 0.7, isotropic=False, device=DEV), Rec("gaussian", 9, 1.4, 3.0, 0.7), 9),
        (D.bivariate_generalized_Gaussian(11, 2.0, 0.9, -0.4, 1.7, isotropic=False, device=DEV),
         Rec("generalized", 11, 2.0, 0.9, -0.4, 1.7), 11),
        (D.bivariate_plateau(5, 1.1, 2.0, 1.0, 0.8, grid=None, isotropic=False, device=DEV),
         Rec("plateau", 5, 1.1, 2.0, 1.0, 0.8), 5),
    ]
    for out, rec, size in cases:
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (size, size)
        check(out[None], R.kernel(rec, size).astype(np.float32)[None], [rec], f"function {rec.kind} {size}")
    # random_mixed_kernels: the record its draws give, then the same kernel
    six = ['iso', 'aniso', 'generalized_iso', 'generalized_aniso', 'plateau_iso', 'plateau_aniso']
    args = (six, [1, 1, 1, 1, 1, 1], 13, (0.3, 4), (0.5, 3), (-np.pi, np.pi), (0.5, 4), (1, 2))
    for seed in range(6):
        random.seed(seed), np.random.seed(seed)
        rec = D.draw_mixed_kernel(*args)
        random.seed(seed), np.random.seed(seed)
        out = D.random_mixed_kernels(*args, noise_range=None, device=DEV)
        assert tuple(out.shape) == (13, 13)
        check(out[None], R.kernel(rec, 13).astype(np.float32)[None], [rec], f"random_mixed_kernels seed {seed}")


SWEEP_N = 1025      # one more than the launch's largest grid (1,024 workgroups): workgroup 0 takes a second trip


@functools.lru_cache(maxsize=None)
def sweep():
    """(records, fp32 reference (n, 21, 21)): every kind, every odd size 3 .. 21, sigma 0.1 .. 5, beta 0.1 .. 8,
    omega_c pi/5 .. pi, theta -pi .. pi; the last record (the second trip's) is a 21 x 21 sinc kernel."""
    from ssl_amd.datapath import KernelRecord
    rng = np.random.default_rng(2323)
    recs = []
    for i in range(SWEEP_N):
        kind = KIND_NAMES[i % 5] if i < SWEEP_N - 1 else "sinc"
        K = int(2 * rng.integers(1, 11) + 1) if i < SWEEP_N - 1 else 21
        sx, sy = np.exp(rng.uniform(np.log(0.1), np.log(5.0), 2))
        if rng.random() < 0.3:
            sy = sx
        recs.append(KernelRecord(kind, K, float(sx), float(sy), float(rng.uniform(-np.pi, np.pi)),
                                 float(np.exp(rng.uniform(np.log(0.1), np.log(8.0)))), float(rng.uniform(np.pi / 5, np.pi))))
    assert {r.size for r in recs} == set(range(3, 22, 2))
    return recs, np.stack([R.kernel(r, 21).astype(np.float32) for r in recs])


def test_sweep_beyond_the_fixture():
    from ssl_amd import datapath
    recs, ref = sweep()
    out = datapath.synth_kernels(recs, 21, DEV)
    assert tuple(out.shape) == (SWEEP_N, 21, 21)
    check(out, ref, recs, "sweep")
    again = datapath.synth_kernels(recs, 21, DEV)
    assert torch.equal(out, again)                       # fixed summation order: bit-reproducible


def test_padding_is_written_and_nothing_else():
    """A direct call into a buffer full of NaN: every element of the n outputs is written, exactly 0 outside the centred
    K x K block, and nothing behind the n-th output is touched; n = 1 and n = 0."""
    from ssl_amd import _lib, datapath
    L = _lib.lib()
    host = datapath.pack_records([datapath.KernelRecord("plateau", 5, 1.3, 0.8, 0.5, 1.5)])
    staged = torch.zeros(host.dtype.itemsize, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for pad in (9, 21):
        buf = torch.full((2, pad, pad), float("nan"), device=DEV)
        with torch.cuda.device(DEV):
            assert L.ssg_synth_kernels(host.ctypes.data, 0, pad, staged.data_ptr(), buf.data_ptr(), stream) == 0
        assert bool(torch.isnan(buf).all())                  # n = 0: nothing launched, nothing written
        with torch.cuda.device(DEV):
            assert L.ssg_synth_kernels(host.ctypes.data, 1, pad, staged.data_ptr(), buf.data_ptr(), stream) == 0
        out = buf.cpu().numpy()
        assert not np.isnan(out[0]).any() and np.isnan(out[1]).all()
        lo = (pad - 5) // 2
        inner = np.zeros((pad, pad), bool)
        inner[lo:lo + 5, lo:lo + 5] = True
        assert (out[0][~inner] == 0).all() and (out[0][inner] > 0).all()
        assert R.within(out[0], R.kernel(datapath.KernelRecord("plateau", 5, 1.3, 0.8, 0.5, 1.5), pad).astype(np.float32),
                        "plateau").all()


def _feed_case(golden):
    from ssl_amd import synth
    opt_ds = eval(str(golden("f23_blur_kernels")["b_all_opt"][0]), {"__builtins__": {}}, {})
    opt = dict(degradation_order="two", scale=4, Use_sharpen=True, Sharpen_before_degra=False,
               resize_prob=[0.2, 0.7, 0.1], resize_range=[0.5, 1.5], gaussian_noise_prob=0.5, noise_range=[1, 30],
               poisson_scale_range=[0.05, 3], gray_noise_prob=0.4, jpeg_range=[30, 95], second_blur_prob=0.8,
               resize_prob2=[0.3, 0.4, 0.3], resize_range2=[0.5, 1.2], gaussian_noise_prob2=0.5, noise_range2=[1, 25],
               poisson_scale_range2=[0.05, 2.5], gray_noise_prob2=0.4, jpeg_range2=[30, 95],
               datasets=dict(train=dict(opt_ds, gt_size=32)))
    B, S = 2, 64
    gt = np.stack([synth.natural_like(2300 + i, S, S, 0.12, 0.04) for i in range(B)]).astype(np.float32)
    mask = np.stack([synth.laplacian_edge_mask(gt[i])[None] for i in range(B)]).astype(np.float32)
    return opt, dict(gt=torch.as_tensor(gt, device=DEV), gt_mask=torch.as_tensor(mask, device=DEV))


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def test_feed_makes_its_own_kernels(golden):
    """Degradation.feed on a dict without kernel1 / kernel2 / sinc_kernel draws and makes them: bit-equal, under the
    same seeds, to feed given the kernels that draw_kernels and synth_kernels produce."""
    from ssl_amd import datapath
    opt, data = _feed_case(golden)
    B = data["gt"].shape[0]
    for seed in (5, 6):
        _seed(seed)
        recs = [datapath.draw_kernels(opt["datasets"]["train"]) for _ in range(B)]
        k = datapath.synth_kernels([r for s in recs for r in s], 9, DEV).view(B, 3, 9, 9)
        want = datapath.Degradation(opt).feed(dict(data, kernel1=k[:, 0], kernel2=k[:, 1], sinc_kernel=k[:, 2]))
        _seed(seed)
        got = datapath.Degradation(opt).feed(dict(data))
        assert got["lq"].shape == (B, 3, 8, 8) and got["gt"].shape == (B, 3, 32, 32)
        for key in ("lq", "gt", "gt_usm", "gt_mask"):
            assert torch.equal(got[key], want[key]), (seed, key)
        assert "kernel1" not in data                                     # the caller's dict is left as it was


@pytest.mark.parametrize("key", ["kernel1", "kernel2", "sinc_kernel"])
def test_feed_refuses_some_but_not_all_kernels(golden, key):
    from ssl_amd import datapath
    opt, data = _feed_case(golden)
    k = torch.zeros(2, 9, 9, device=DEV)
    k[:, 4, 4] = 1
    with pytest.raises(ValueError, match="together or none"):
        datapath.Degradation(opt).feed(dict(data, **{key: k}))
    two = dict(data, kernel1=k, kernel2=k, sinc_kernel=k)
    del two[key]
    with pytest.raises(ValueError, match="together or none"):
        datapath.Degradation(opt).feed(two)
