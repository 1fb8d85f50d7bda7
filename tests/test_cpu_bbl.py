"""BebyGAN's best-buddy loss and flat mask without a GPU: the fp64 restatement of the contract (tests/bbl_reference.py)
that the GPU tests use reproduces the reference's own outputs (tests/golden/f19_bbl.npz), the new symbols are exported,
the C ABI refuses bad arguments before it launches anything, and the Python layer refuses what lies outside the native
domain."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bbl_reference as R

BBL_SYMBOLS = ("ssg_bbl_workspace_bytes", "ssg_bbl_search", "ssg_bbl_loss", "ssg_flat_mask")


def _cases(golden):
    z = golden("f19_bbl")
    for i in range(int(z["n_cases"])):
        yield i, {k[len(f"c{i}_"):]: z[k] for k in z.files if k.startswith(f"c{i}_")}


def test_f19_covers_what_it_must(golden):
    cases = dict(_cases(golden))
    assert any(c["x"].shape[2] % 2 and c["x"].shape[2] % 3 and c["x"].shape[3] % 3 and c["x"].shape[3] % 4
               for c in cases.values())
    assert any(float(c["alpha"]) != 1 and float(c["beta"]) != 1 for c in cases.values())
    assert any(c["x"].shape[1] == 1 for c in cases.values())


def test_bicubic_levels_are_torchs(golden):
    """The fixed-tap pyramid of the restatement is F.interpolate(.., 'bicubic', align_corners=False) in fp64."""
    for _, c in _cases(golden):
        g = torch.from_numpy(c["gt"]).double()
        for shift, f in ((1, 0.5), (2, 0.25)):
            want = F.interpolate(g, scale_factor=f, mode='bicubic', align_corners=False)
            got = R.half_or_quarter(g, shift)
            assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-14


def test_restatement_reproduces_f19(golden):
    """sel_p2 within 1e-6 for every row the fp64 scores decide (gap to the best candidate of other content > tau);
    loss and gradient, evaluated at the indices the reference's sel_p2 implies, within 1e-6 of their maximum."""
    decided_total = rows_total = 0
    for i, c in _cases(golden):
        x, gt = torch.from_numpy(c["x"]), torch.from_numpy(c["gt"])
        alpha, beta = float(c["alpha"]), float(c["beta"])
        sc, p1, cand = R.scores(x, gt, alpha, beta)
        assert torch.equal(p1.float(), torch.from_numpy(c["p1"])), i
        best = R.argmin_lowest(sc)
        gap = R.gap_to_distinct(sc, cand, best)
        decided = gap > R.tau(cand.shape[-1], alpha, beta, x, gt)
        sel = cand.gather(1, best[..., None].expand(-1, -1, cand.shape[-1]))
        err = (sel - torch.from_numpy(c["sel_p2"]).double()).abs().amax(-1)
        assert float(err[decided].max()) <= 1e-6, (i, float(err[decided].max()))
        decided_total += int(decided.sum())
        rows_total += decided.numel()
        # the reference's own picks: the candidate its sel_p2 row is (nearest in content)
        ref_ind = torch.cdist(torch.from_numpy(c["sel_p2"]).double(), cand).argmin(-1)
        loss, grad, _ = R.loss_and_grad(x, cand, ref_ind)
        assert abs(float(loss) - float(c["loss"])) <= 1e-6 * max(float(c["loss"]), 1e-30), i
        gmax = float(np.abs(c["grad"]).max())
        assert float((grad - torch.from_numpy(c["grad"]).double()).abs().max()) <= 1e-6 * gmax, i
    assert decided_total >= 0.9 * rows_total, (decided_total, rows_total)


def test_flat_mask_restatement_reproduces_f19_bit_for_bit(golden):
    z = golden("f19_bbl")
    img = torch.from_numpy(z["m_img"])
    for k in (11, 3):
        std = R.flat_std(img, k)
        assert int(((std - 0.025).abs() <= 1e-6).sum()) == 0
        assert torch.equal((std < 0.025).float(), torch.from_numpy(z[f"m_mask_k{k}"])), k
    n = 0
    for i, c in _cases(golden):
        if "mask" in c:
            n += 1
            assert torch.equal((R.flat_std(torch.from_numpy(c["gt"]), 11) < 0.025).float(), torch.from_numpy(c["mask"])), i
    assert n >= 3


def test_bbl_symbols_are_exported():
    from ssl_amd import _lib
    import ssl_amd.losses as losses
    _lib.build()
    L = ctypes.CDLL(_lib.SO_PATH)
    hdr = open(_lib.HEADER).read()
    for name in BBL_SYMBOLS:
        assert hasattr(L, name) and name in _lib.PROTOTYPES and f"{name}(" in hdr, name
    for name in ("BBL", "BestBuddyLoss", "get_flat_mask"):
        assert callable(getattr(losses, name)), name
    b = losses.BBL()
    assert (b.alpha, b.beta, b.ksize, b.pad, b.stride, b.dist_norm) == (1.0, 1.0, 3, 0, 3, 'l2')
    m = losses.BestBuddyLoss()
    assert (m.loss_weight, m.reduction, m.alpha, m.beta) == (1.0, 'mean', 1.0, 1.0)
    assert _lib.lib().ssg_abi_version() == 6
    # the training size: operands and partials, a few tens of MB -- not the 1.41 GB of one score matrix
    nb = _lib.lib().ssg_bbl_workspace_bytes(16, 3, 192, 192, 3, 3)
    assert 16 * (4096 + 5376) * 28 * 4 <= nb <= 64 << 20


def test_bbl_argument_checks_need_no_gpu():
    """SSG_E_BADARG (-1), SSG_E_TOOLARGE (-2), SSG_E_WORKSPACE (-3), SSG_E_IMAGESMALL (-4), SSG_E_ALIGN (-5): all
    decided before a launch (the pointers below are never dereferenced)."""
    from ssl_amd import _lib
    L = _lib.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(24)
    big = 1 << 40

    def search(x=one, B=2, C=3, H=24, W=24, k=3, s=3, a=1.0, b=1.0, ind=one, ws=one, nb=big):
        return L.ssg_bbl_search(x, one, B, C, H, W, k, s, a, b, ind, None, None, ws, nb, None)

    def loss(x=one, B=2, C=3, H=24, W=24, k=3, s=3, a=1.0, b=1.0, out=one, ws=one, nb=big):
        return L.ssg_bbl_loss(x, one, B, C, H, W, k, s, a, b, 1.0, 1, out, None, None, ws, nb, None)

    for f in (search, loss):
        assert f(x=None) == -1 and f(ws=None) == -1 and f(B=0) == -1 and f(C=0) == -1 and f(k=0) == -1
        assert f(s=2) == -1 and f(a=-1.0) == -1 and f(a=0.0, b=0.0) == -1 and f(b=float('nan')) == -1
        assert f(k=4, s=4, H=64, W=64) == -2 and f(C=4) == -2 and f(B=70000) == -2          # d = 48, 36
        assert f(H=11) == -4 and f(W=11) == -4 and f(k=5, s=5, C=1, H=19, W=40) == -4
        assert f(H=12, W=12, nb=L.ssg_bbl_workspace_bytes(2, 3, 12, 12, 3, 3) - 1) == -3 and f(nb=16) == -3
        assert f(ws=odd) == -5
    assert search(ind=None) == -1 and loss(out=None) == -1
    assert L.ssg_bbl_workspace_bytes(2, 3, 11, 24, 3, 3) == 0 and L.ssg_bbl_workspace_bytes(2, 3, 12, 12, 3, 3) > 0

    def mask(img=one, B=1, H=16, W=16, k=11, out=one):
        return L.ssg_flat_mask(img, B, H, W, k, 0.025, out, None)

    assert mask(img=None) == -1 and mask(out=None) == -1 and mask(B=0) == -1 and mask(H=0) == -1
    for k in (10, 0, -3, 1, 2):
        assert mask(k=k) == -1, k
    assert mask(k=17) == -2
    assert mask(H=5) == -4 and mask(W=5) == -4 and mask(k=3, W=1) == -4


def test_outside_the_native_domain_raises_not_implemented():
    from ssl_amd.losses import BBL, BestBuddyLoss
    for kw, word in ((dict(dist_norm='l1'), "l2"), (dict(pad=1), "pad"), (dict(ksize=3, stride=2), "stride"),
                     (dict(ksize=5, stride=3), "stride")):
        with pytest.raises(NotImplementedError, match=word):
            BBL(**kw)
    with pytest.raises(NotImplementedError, match="stride"):
        BestBuddyLoss(ksize=3, stride=1)
    with pytest.raises(ValueError):
        BestBuddyLoss(reduction='none')
    assert BBL(alpha=0.5, beta=2.0, ksize=2, stride=4).stride == 4
