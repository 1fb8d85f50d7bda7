"""The diffusion kernels (ssl_amd/csrc/ssg_diffusion.hip) through the C ABI on sentinel-filled memory: every output and
workspace lies inside a larger buffer filled with a sentinel, at an offset of 0 to 3 floats of its own, and after the call
the bytes in front of and behind it must still be the sentinel while what was written is the oracle's.  A kernel that
stored one element past a chunk's tail, a sample's end or a tile's edge would show here."""
import pytest
import torch

import diffusion_cases as C
import diffusion_reference as R
from test_gpu_diffusion import DEV, _need_gpu, schedule

pytestmark = pytest.mark.gpu
SENTINEL = 0x7FC0DEAD                                                           # a NaN with a payload, as int32
GUARD = 64                                                                      # words on either side


class Guarded:
    """`count` words (4 bytes; `width` 2: 8-byte elements) at `offset` words past the front guard."""

    def __init__(self, count, offset=0, dtype=torch.float32):
        self.width = 2 if dtype in (torch.float64, torch.int64) else 1
        self.words, self.offset, self.dtype = count * self.width, offset * self.width, dtype
        self.buf = torch.full((GUARD + self.offset + self.words + GUARD + 3,), SENTINEL, dtype=torch.int32, device=DEV)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * (GUARD + self.offset)

    def inside(self):
        return self.buf[GUARD + self.offset:GUARD + self.offset + self.words].view(self.dtype)

    def guards_intact(self):
        lo, hi = GUARD + self.offset, GUARD + self.offset + self.words
        return bool((self.buf[:lo] == SENTINEL).all()) and bool((self.buf[hi:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


def _at(view, offset):
    flat = torch.empty(view.numel() + 3, dtype=view.dtype, device=DEV)
    out = flat[offset:offset + view.numel()].view(view.shape)
    out.copy_(view)
    return out


def _launch(fn, *args):
    from ssl_amd import _gpu
    _gpu.launch(DEV, fn, *args)
    torch.cuda.synchronize()


@pytest.mark.parametrize("B", C.BATCHES)
@pytest.mark.parametrize("which", range(6))
def test_per_sample_kernels_write_their_outputs_only(B, which):
    _need_gpu()
    from ssl_amd import _lib
    L = _lib.lib()
    n = C.sample_counts(L.ssg_diff_chunk())[which]
    s, tab = schedule()
    seed = 200 + 10 * B + which
    cpu = [v.view(B, 1, 1, n) for v in C.sample_inputs(B, n, seed, specials=False)]
    a, b, z = cpu
    ga, gb, gz = (_at(v, (seed + 2 * j) % 4) for j, v in enumerate(cpu))
    t = C.timesteps(B, 1000, seed)
    gt = t.to(DEV)
    T = 1000
    # combine, clamped
    out = Guarded(B * n, (seed + 1) % 4)
    _launch(L.ssg_diff_combine, ga.data_ptr(), gb.data_ptr(), gt.data_ptr(), s.sqrt_recip_alphas_cumprod.data_ptr(),
            s.sqrt_recipm1_alphas_cumprod.data_ptr(), T, B, n, 1, 1, -0.5, 0.75, out.ptr)
    want = R.combine(tab["sqrt_recip_alphas_cumprod"], a, tab["sqrt_recipm1_alphas_cumprod"], b, t, True, (-0.5, 0.75))
    assert out.guards_intact() and R.same_bits(out.inside().view(B, 1, 1, n), want) == 0
    # p_sample with x0
    out, x0 = Guarded(B * n, (seed + 2) % 4), Guarded(B * n, (seed + 3) % 4)
    _launch(L.ssg_diff_p_sample, ga.data_ptr(), gb.data_ptr(), gz.data_ptr(), gt.data_ptr(),
            s.sqrt_recip_alphas_cumprod.data_ptr(), s.sqrt_recipm1_alphas_cumprod.data_ptr(),
            s.posterior_mean_coef1.data_ptr(), s.posterior_mean_coef2.data_ptr(), s.sigma.data_ptr(), T, B, n, 0, 1,
            out.ptr, x0.ptr)
    want, want0 = R.p_sample(tab, a, b, t, z, "eps", True, return_x0=True)
    assert out.guards_intact() and x0.guards_intact()
    assert R.same_bits(out.inside().view(B, 1, 1, n), want) == 0 and R.same_bits(x0.inside().view(B, 1, 1, n), want0) == 0
    # the criterion: partials, the finishing outputs, the gradient
    nbytes = L.ssg_diff_workspace_bytes(B, n)
    chunks = nbytes // 8
    assert chunks == B * (-(-n // L.ssg_diff_chunk()))
    ws = Guarded(chunks, 0, torch.float64)
    _launch(L.ssg_diff_loss_sums, ga.data_ptr(), gb.data_ptr(), B, n, 1, ws.ptr, nbytes)
    assert ws.guards_intact() and bool(torch.isfinite(ws.inside()).all())
    logvar = C.logvar_table(T, seed)
    glv = logvar.to(DEV)
    S, scal, coef, dlv = (Guarded(k, 0, torch.float64) for k in (B, 4, B, T))
    before = ws.buf.clone()
    _launch(L.ssg_diff_loss_finish, ws.ptr, nbytes, gt.data_ptr(), None, glv.data_ptr(), s.lvlb_weights.data_ptr(), T, B, n,
            1.0, 0.5, S.ptr, scal.ptr, coef.ptr, dlv.ptr)
    assert torch.equal(ws.buf, before) and all(g.guards_intact() for g in (S, scal, coef, dlv))
    ref = R.criterion64(a, b, z, t, tab, logvar, "l2", 1.0, 0.5)
    b_scal, b_grad, per, Rm = R.criterion_bounds(ref, "l2", 1.0, 0.5)
    assert R.share(S.inside(), ref["S"], Rm * ref["S"]) <= 1.0
    assert all(R.share(scal.inside()[k], ref["scalars"][k], b_scal[k]) <= 1.0 for k in range(4))
    assert R.share(dlv.inside(), ref["grad_logvar"], R.logvar_bound(per, t, T)) <= 1.0
    # without the nullable output nothing of it is written
    dlv2, S2, scal2, coef2 = Guarded(T, 0, torch.float64), Guarded(B, 0, torch.float64), Guarded(4, 0, torch.float64), \
        Guarded(B, 0, torch.float64)
    _launch(L.ssg_diff_loss_finish, ws.ptr, nbytes, gt.data_ptr(), None, glv.data_ptr(), s.lvlb_weights.data_ptr(), T, B, n,
            1.0, 0.5, S2.ptr, scal2.ptr, coef2.ptr, None)
    assert dlv2.untouched() and torch.equal(S2.inside(), S.inside()) and torch.equal(coef2.inside(), coef.inside())
    g = torch.ones(1, device=DEV)
    grad = Guarded(B * n, (seed + 3) % 4)
    _launch(L.ssg_diff_loss_grad, ga.data_ptr(), gb.data_ptr(), None, None, None, 0, g.data_ptr(), coef.ptr, B, n, 1, grad.ptr)
    assert grad.guards_intact() and R.share(grad.inside().view(B, 1, 1, n), ref["grad_pred"], b_grad) <= 1.0
    # the same without grad_x0 for l1 (coef does not depend on the kind: the l2 call's serves)
    ref1 = R.criterion64(a, b, z, t, tab, logvar, "l1", 1.0, 0.5)
    grad = Guarded(B * n, (seed + 2) % 4)
    _launch(L.ssg_diff_loss_grad, ga.data_ptr(), gb.data_ptr(), None, None, None, 0, g.data_ptr(), coef.ptr, B, n, 0, grad.ptr)
    assert grad.guards_intact()
    assert R.share(grad.inside().view(B, 1, 1, n), ref1["grad_pred"], R.criterion_bounds(ref1, "l1", 1.0, 0.5)[1]) <= 1.0
    gx0 = C.sample_inputs(B, n, seed + 50, specials=False, count=1)[0].view(B, 1, 1, n)
    ggx0 = _at(gx0, (seed + 1) % 4)
    ref = R.criterion64(a, b, z, t, tab, logvar, "l2", 1.0, 0.5, grad_x0=gx0)
    _, b_grad, _, _ = R.criterion_bounds(ref, "l2", 1.0, 0.5, grad_x0=gx0)
    grad = Guarded(B * n, seed % 4)
    _launch(L.ssg_diff_loss_grad, ga.data_ptr(), gb.data_ptr(), ggx0.data_ptr(), gt.data_ptr(),
            s.sqrt_recipm1_alphas_cumprod.data_ptr(), T, g.data_ptr(), coef.ptr, B, n, 1, grad.ptr)
    assert grad.guards_intact() and R.share(grad.inside().view(B, 1, 1, n), ref["grad_pred"], b_grad) <= 1.0


@pytest.mark.parametrize("case", C.CANVAS[:6])
@pytest.mark.parametrize("B", C.CANVAS_BATCHES)
def test_canvas_kernels_write_their_outputs_only(case, B):
    _need_gpu()
    from ssl_amd import _lib, diffusion
    L = _lib.lib()
    ts, overlap, h, w = case
    tiles, grid = diffusion.canvas_tiles(h, w, ts, overlap)
    x, sc = C.canvas_inputs(case, B)
    gx = _at(x, 1)
    table = torch.tensor([(oy, ox, k * B) for k, (oy, ox) in enumerate(tiles)], dtype=torch.int32, device=DEV)
    count = len(tiles) * B * C.CANVAS_C * ts * ts
    out = Guarded(count, 3)
    _launch(L.ssg_diff_canvas_gather, gx.data_ptr(), table.data_ptr(), len(tiles), B, C.CANVAS_C, h, w, ts, out.ptr)
    want = R.canvas_gather(x, tiles, ts)
    assert out.guards_intact() and R.same_bits(out.inside().view(want.shape), want) == 0
    preds = C.stand_in_network(want, R.canvas_gather(sc, tiles, ts))
    gp = _at(preds, 2)
    weights = R.gaussian_weights(ts, ts)
    gw = weights.to(DEV)
    canvas = Guarded(x.numel(), 1)
    _launch(L.ssg_diff_canvas_stitch, gp.data_ptr(), len(tiles) * B, 1, table.data_ptr(), len(tiles), gw.data_ptr(), 0, 0,
            B, C.CANVAS_C, h, w, ts, canvas.ptr)
    assert canvas.guards_intact()
    assert R.same_bits(canvas.inside().view(x.shape), R.canvas_stitch(preds, tiles, x.shape, weights)) == 0
    # records that leave the canvas or the prediction tensor are skipped: nothing outside is read or written
    bad = table.clone()
    bad[0] = torch.tensor([h - ts + 1, 0, 0], dtype=torch.int32)
    if len(tiles) > 1:
        bad[1] = torch.tensor([0, 0, len(tiles) * B], dtype=torch.int32)
    keep = [k for k in range(len(tiles)) if k >= 2]
    out = Guarded(count, 0)
    _launch(L.ssg_diff_canvas_gather, gx.data_ptr(), bad.data_ptr(), len(tiles), B, C.CANVAS_C, h, w, ts, out.ptr)
    got = out.inside().view(want.shape)
    assert out.guards_intact() and bool((got[:B].view(torch.int32) == SENTINEL).all())
    canvas = Guarded(x.numel(), 0)
    _launch(L.ssg_diff_canvas_stitch, gp.data_ptr(), len(tiles) * B, 1, bad.data_ptr(), len(tiles), gw.data_ptr(), 0, 0,
            B, C.CANVAS_C, h, w, ts, canvas.ptr)
    expect = R.canvas_stitch(preds, tiles, x.shape, weights, order=keep)       # (0 / 0 where nothing is left: NaN)
    assert canvas.guards_intact() and R.same_bits(canvas.inside().view(x.shape), expect) == 0
