"""The GAN criteria's restatement and bound (tests/gan_reference.py) against the reference's recorded results
(tests/golden/f32_gan.npz, written by make_golden_gan.py) and against fp64 autograd through the torch expressions, and
what of ssl_amd.losses.gan_loss and its C ABI can be checked without a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gan_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f32_gan.npz")
PLAIN, REL = R.fixture_plain_cases(), R.fixture_rel_cases()
MULTI = (("vanilla", True, False, False), ("hinge", False, True, False), ("vanilla", True, False, True))


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def _crit(source, gan_type, labels):
    from ssl_amd.losses import GANLoss
    if source == "basicsr":
        return GANLoss(gan_type, labels[0], labels[1], loss_weight=R.FIXTURE_WEIGHT)
    return GANLoss(gan_type.upper(), labels[0], labels[1])       # KAIR lowercases the name and has no weight


def _weight(source, disc):
    return R.FIXTURE_WEIGHT if source == "basicsr" and not disc else 1.0


def _rel_inputs(golden, source):
    return (golden["real"], golden["fake"]) if source == "basicsr" else (golden["kreal"], golden["kfake"])


def _rel_module(crit, form, real, fake, dtype):
    need = R.rel_needs(form)
    a, b = real.to(dtype).clone().requires_grad_(need[0]), fake.to(dtype).clone().requires_grad_(need[1])
    loss = R.rel_form(form, a, b, crit.relativistic_term, crit.relativistic_generator)
    loss.backward()
    return loss.detach(), a.grad if need[0] else torch.zeros_like(a), b.grad if need[1] else torch.zeros_like(b)


def _rel_restated(source, gan_type, labels, form, real, fake, exact=False):
    """(L, dL/dreal, dL/dfake, bounds of the three for a result computed with an fp32 mean)."""
    w = _weight(source, form.startswith("disc"))
    if form.startswith("gen"):
        sa, sb = R.spec(gan_type, False, False, *labels), R.spec(gan_type, True, False, *labels)
        L, gr, gf = R.relativistic_generator(real, fake, sa, sb, w, exact=exact)
        bl, br, bf = R.generator_bounds(real, fake, sa, sb, w, reference_mean=True)
        need = R.rel_needs(form)
        return L, gr * need[0], gf * need[1], bl, br, bf
    pred, other, is_real = (real, fake, True) if form == "disc_real" else (fake, real, False)
    sp = R.spec(gan_type, is_real, True, *labels)
    L, gp, _, _ = R.relativistic_term(pred, other, sp, w, 0.5, exact=exact)
    bl, bp, _ = R.term_bounds(pred, other, sp, w, 0.5, reference_mean=True)
    zero = torch.zeros(tuple(other.shape), dtype=torch.float64)
    out = (L * 0.5, gp, zero, bl * 0.5 + R.U * abs(float(L)), bp, zero + R.TINY)
    return out if form == "disc_real" else (out[0], out[2], out[1], out[3], out[5], out[4])


def test_fixture_holds_numbers_only_and_stays_small(golden):
    assert all(v.dtype == torch.float32 for v in golden.values())
    assert os.path.getsize(GOLDEN) < 128 * 1024
    assert len(PLAIN) == 60 and len(REL) == 48
    assert sum(1 for k in golden if k.endswith("_loss")) == len(PLAIN) + len(REL) + len(MULTI)
    for k, v in R.fixture_inputs().items():
        assert torch.equal(golden[k], v), k
    assert golden["real"].numel() != golden["fake"].numel()


@pytest.mark.parametrize("n", range(len(PLAIN)))
def test_plain_restatement_module_and_reference(golden, n):
    """One plain case: the restatement equals fp64 autograd through the module's torch expressions to 1e-12, the
    reference's recorded fp32 result lies inside the bound, and the module on the CPU equals it bit for bit."""
    source, gan_type, real, disc, labels = PLAIN[n]
    crit, w, sp = _crit(source, gan_type, labels), _weight(source, disc), R.spec(gan_type, real, disc, *labels)
    x = golden["x"]
    want_l, want_g = R.plain(x, sp, w)
    # fp64 autograd; its labels are the fp64 values, the restatement's the fp32 ones the kernels are given
    sp64 = (sp[0], sp[1], float((labels[0] if real else labels[1])) if sp[0] in (R.BCE, R.LS) else 0.0)
    a = x.double().requires_grad_(True)
    l64 = crit(a, real, disc)
    l64.backward()
    r_l, r_g = R.plain(x, sp64, w)
    d = R.delta(x)
    # (torch's softplus returns z beyond 20, in fp64 too: the restatement is the function, CUT apart there)
    cut = R.CUT * (sp[1] * d > 20).double() if sp[0] == R.SOFTPLUS else torch.zeros_like(d)
    assert abs(float(l64.detach()) - float(r_l)) <= 1e-12 * abs(float(r_l)) + w * float(cut.mean())
    assert bool(((a.grad - r_g).abs() <= 1e-12 * float(r_g.abs().max()) + w * cut / d.numel()).all())
    shares = (R.share(golden[f"p{n}_loss"], want_l, R.loss_bound(d, sp, w)),
              R.share(golden[f"p{n}_grad"], want_g, R.grad_bound(d, sp, w / d.numel())))
    print(f"plain {n} {source} {gan_type} real={real} disc={disc} labels={labels}: the reference uses "
          f"{shares[0]:.3e} / {shares[1]:.3e} of the loss / gradient bound")
    assert max(shares) <= 1.0
    b = x.clone().requires_grad_(True)
    loss = crit(b, real, disc)
    loss.backward()
    assert loss.grad_fn is not None and "PlainCriterion" not in type(loss.grad_fn).__name__
    assert torch.equal(loss.detach(), golden[f"p{n}_loss"]) and torch.equal(b.grad, golden[f"p{n}_grad"])


@pytest.mark.parametrize("n", range(len(REL)))
def test_relativistic_restatement_module_and_reference(golden, n):
    source, gan_type, labels, form = REL[n]
    crit = _crit(source, gan_type, labels)
    real, fake = _rel_inputs(golden, source)
    if labels == R.LABELS[0]:          # (labels 0.9 / 0.1 are not fp64 values of their fp32 roundings: bound only)
        l64, gr64, gf64 = _rel_module(crit, form, real, fake, torch.float64)
        L, gr, gf = _rel_restated(source, gan_type, labels, form, real, fake, exact=True)[:3]
        scale = max(float(gr.abs().max()), float(gf.abs().max()))
        assert abs(float(l64) - float(L)) <= 1e-12 * max(abs(float(L)), 1e-300)
        assert float((gr64 - gr).abs().max()) <= 1e-12 * scale and float((gf64 - gf).abs().max()) <= 1e-12 * scale
    L, gr, gf, bl, br, bf = _rel_restated(source, gan_type, labels, form, real, fake)
    shares = (R.share(golden[f"r{n}_loss"], L, bl), R.share(golden[f"r{n}_greal"], gr, br),
              R.share(golden[f"r{n}_gfake"], gf, bf))
    print(f"relativistic {n} {source} {gan_type} labels={labels} {form}: the reference uses {shares[0]:.3e} / "
          f"{shares[1]:.3e} / {shares[2]:.3e} of the loss / grad_real / grad_fake bound")
    assert max(shares) <= 1.0
    l32, gr32, gf32 = _rel_module(crit, form, real, fake, torch.float32)
    assert torch.equal(l32, golden[f"r{n}_loss"])
    assert torch.equal(gr32, golden[f"r{n}_greal"]) and torch.equal(gf32, golden[f"r{n}_gfake"])


@pytest.mark.parametrize("n", range(len(MULTI)))
def test_multiscale_restatement_module_and_reference(golden, n):
    from ssl_amd.losses import MultiScaleGANLoss
    gan_type, real, disc, nested = MULTI[n]
    crit = MultiScaleGANLoss(gan_type, loss_weight=R.FIXTURE_WEIGHT)
    w, sp = _weight("basicsr", disc), R.spec(gan_type, real, disc)
    scales = [golden["s0"], golden["s1"], golden["s2"]]
    leaves = [t.clone().requires_grad_(True) for t in scales]
    arg = [[golden["x"], leaves[0]], [golden["real"], leaves[1]], [leaves[2]]] if nested else leaves
    loss = crit(arg, real, disc)
    loss.backward()
    assert torch.equal(loss.detach(), golden[f"m{n}_loss"])
    L, grads = R.multiscale(scales, sp, w)
    bound = sum(R.loss_bound(R.delta(t), sp, w) for t in scales) / 3 + 4 * R.U * abs(float(L))
    assert R.share(golden[f"m{n}_loss"], L, bound) <= 1.0
    for k, (leaf, g, t) in enumerate(zip(leaves, grads, scales)):
        assert torch.equal(leaf.grad, golden[f"m{n}_g{k}"])
        assert R.share(leaf.grad, g, R.grad_bound(R.delta(t), sp, w / (3 * t.numel()))) <= 1.0
    single = crit(golden["s0"], real, disc)                    # a tensor goes to GANLoss unchanged
    assert abs(float(single) - float(R.plain(golden["s0"], sp, w)[0])) <= R.loss_bound(R.delta(golden["s0"]), sp, w)


def test_both_naming_schemes_resolve_and_unknown_names_raise():
    from ssl_amd.losses import GANLoss, MultiScaleGANLoss
    from ssl_amd.losses import gan_loss as M
    kinds = {"vanilla": M.BCE, "gan": M.BCE, "ragan": M.BCE, "RaGAN": M.BCE, "lsgan": M.LS, "LSGAN": M.LS,
             "wgan": M.LINEAR, "wgan_softplus": M.SOFTPLUS, "softplusgan": M.SOFTPLUS, "hinge": M.HINGE}
    for name, kind in kinds.items():
        crit = GANLoss(name, 0.9, 0.1, loss_weight=0.3)
        assert crit.gan_type == name and (crit.real_label_val, crit.fake_label_val, crit.loss_weight) == (0.9, 0.1, 0.3)
        got = crit._spec(True, True)
        assert got[0] == kind and got == R.spec(name.lower(), True, True, 0.9, 0.1)[:2] + (got[2],)
        assert got[2] == (0.9 if kind in (M.BCE, M.LS) else 0.0)
        assert crit._spec(False, False)[:2] == R.spec(name.lower(), False, False)[:2]
    assert GANLoss("hinge")._spec(True, False) == (M.LINEAR, -1.0, 0.0) == GANLoss("hinge")._spec(False, False)
    assert (M.BCE, M.LS, M.LINEAR, M.SOFTPLUS, M.HINGE) == (R.BCE, R.LS, R.LINEAR, R.SOFTPLUS, R.HINGE)
    for name in ("", "dcgan", "vanila", "soft plus", None):
        for cls in (GANLoss, MultiScaleGANLoss):
            with pytest.raises(NotImplementedError):
                cls(name)


def test_loss_weight_is_the_generators_alone():
    from ssl_amd.losses import GANLoss
    x = R.logits((3, 1, 4, 4), 9)
    for name in R.BASICSR_TYPES:
        half, one = GANLoss(name, loss_weight=0.5), GANLoss(name, loss_weight=1.0)
        assert torch.equal(half(x, True, is_disc=True), one(x, True, is_disc=True))
        assert torch.equal(half(x, True), one(x, True) * 0.5)


# -------------------------------------------------------------------------------------------------- host checks ---
NAMES = ("ssg_gan_workspace_bytes", "ssg_gan_grid_cap", "ssg_gan_sums", "ssg_gan_grad")
FAKE = [ctypes.c_void_p(k << 20) for k in range(1, 6)]     # non-null, aligned addresses a refused call never touches


def _declaration(hdr, name):
    m = re.search(r"^(?:int|size_t) " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
    assert m, name
    text = re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " "))
    return [a.strip() for a in text.split(",") if a.strip() != "void"]


def test_symbols_exported_declared_and_bound():
    from ssl_amd import _lib, losses
    from ssl_amd.losses import gan_loss as M
    _lib.build()
    L = _lib.lib()
    hdr = open(_lib.HEADER).read()
    kinds = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
    for name in NAMES:
        assert hasattr(L, name)
        res, args = _lib.PROTOTYPES[name]
        decl = _declaration(hdr, name)
        assert len(decl) == len(args), name
        for d, a in zip(decl, args):
            want = ctypes.c_void_p if ("*" in d or d.startswith("ssg_stream_t")) else kinds[d.split()[0]]
            assert a is want, (name, d)
        assert res is (ctypes.c_size_t if name.endswith("_bytes") else ctypes.c_int)
    assert L.ssg_abi_version() == 6
    assert [_lib.CONSTANTS["SSG_GAN_" + k] for k in ("BCE", "LS", "LINEAR", "SOFTPLUS", "HINGE")] == [0, 1, 2, 3, 4]
    for name in ("GANLoss", "MultiScaleGANLoss"):
        assert getattr(losses, name) is getattr(M, name) and name in M.__all__
    assert issubclass(M.MultiScaleGANLoss, M.GANLoss)


def test_workspace_follows_the_grid_cap_and_the_trip_shape_follows_both():
    """gan_cases.py's largest shape is computed from the exported cap: every workgroup makes a second trip and a tail
    of five elements remains."""
    from ssl_amd import _lib
    import gan_cases as C
    L = _lib.lib()
    cap = L.ssg_gan_grid_cap()
    assert cap >= 1 and L.ssg_gan_workspace_bytes() == 2 * 8 * cap
    assert C.trip_elements(cap) == cap * C.WORKGROUP * C.PER_THREAD + 5
    assert C.trip_elements(cap) * 4 <= 64 << 20                  # a few megabytes: the test stays quick


def test_c_abi_refuses_before_any_launch():
    from ssl_amd import _lib
    L = _lib.lib()
    BAD = -1
    x, shift, work, sums, coef = FAKE
    ok = dict(n=70, kind=0, sign=1.0, label=1.0)

    def sums_call(x=x, work=work, sums=sums, shift=shift, **kw):
        a = dict(ok, **kw)
        return L.ssg_gan_sums(x, a["n"], a["kind"], a["sign"], a["label"], shift, work, sums, None)

    def grad_call(x=x, coef=coef, grad=work, shift=shift, **kw):
        a = dict(ok, **kw)
        return L.ssg_gan_grad(x, a["n"], a["kind"], a["sign"], a["label"], shift, coef, grad, None)

    for call in (sums_call, grad_call):
        assert call(x=None) == BAD
        assert call(n=0) == BAD
        for kind in (-1, 5, 17):
            assert call(kind=kind) == BAD
        for sign in (0.0, 2.0, -0.5, float("nan"), float("inf")):
            assert call(sign=sign) == BAD
    assert sums_call(work=None) == BAD and sums_call(sums=None) == BAD
    assert grad_call(coef=None) == BAD and grad_call(grad=None) == BAD
    assert sums_call(x=ctypes.c_void_p((1 << 20) + 2)) == -5 and grad_call(grad=ctypes.c_void_p((3 << 20) + 2)) == -5
    assert sums_call(sums=ctypes.c_void_p((4 << 20) + 4)) == -5 and grad_call(coef=ctypes.c_void_p((5 << 20) + 4)) == -5
    # two things wrong at once: the logits (null, n, kind, sign, then their alignment) are judged before the other
    # pointers, and a null pointer before any of those is measured
    odd, half = ctypes.c_void_p((1 << 20) + 2), ctypes.c_void_p((4 << 20) + 4)
    for call in (sums_call, grad_call):
        assert call(x=odd, kind=5) == BAD and call(x=odd, n=0) == BAD and call(x=odd, sign=0.0) == BAD
    assert sums_call(x=odd, work=None) == -5 and sums_call(x=odd, sums=None) == -5
    assert grad_call(x=odd, coef=None) == -5 and grad_call(x=odd, grad=None) == -5
    assert sums_call(work=None, sums=half) == BAD and sums_call(work=half, sums=None) == BAD
    assert grad_call(coef=None, grad=odd) == BAD and grad_call(coef=half, grad=None) == BAD
