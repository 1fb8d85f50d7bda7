"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

The branch-aware comparison of a DiffJPEG(differentiable=False) output with oracle/datapath_oracle.diffjpeg, for
tests/test_cpu_jpeg.py, tests/test_gpu_jpeg.py and the JPEG parts of tests/test_gpu_parity.py.

torch.round of a quotient that fp32 puts on the other side of k + 1/2 than fp64 moves a whole 8 x 8 block by one
quantisation step; neither result is wrong.  Instead of leaving such blocks out, the comparison lets exactly those
roundings go either way and nothing else:

  window     per sample, max(2e-4, 4 x max |quot32 - quot64|) with both quotient sets from the oracle (evaluated in
             np.float32 and np.float64), never from the code under test; the 4 x is grad_tol_from_oracle's margin.
  undecided  a coefficient whose fp64 quotient lies inside the window around k + 1/2.  Every other coefficient is
             decided and must round as fp64 does.
  match      per 16 x 16 macroblock (4 luma blocks + Cb + Cr, what one wave of jpeg_kernel computes): SOME assignment of
             its undecided roundings brings every pixel of the macroblock, all three channels, cropped to H x W,
             within the bound.  One assignment serves the whole macroblock, so a Cb or Cr choice is shared by the four
             luma blocks.  Macroblocks do not interact, so the 2^n assignments are walked per macroblock, on the
             oracle run on that macroblock's pixels alone.
  bound      3e-6, the project's F14 bound (the reference's own fp32 output is within 4.4e-7 of a matching assignment
             on every case of tests/jpeg_cases.py, tests/test_cpu_jpeg.py).
  cap        at most 8 undecided coefficients in a macroblock.  It is a condition on the INPUT: JpegOracle refuses an
             input with a macroblock over it (tests/test_cpu_jpeg.py asserts that no case has one), so that no
             macroblock is ever left out of a comparison.
"""
import numpy as np

from oracle import datapath_oracle as dp

BOUND = 3e-6
CAP = 8
MIN_WINDOW = 2e-4
WINDOW_MARGIN = 4.0


def _mb_max(a, s):
    """(B, h, w) -> (B, h / s, w / s): maximum over s x s tiles (NaN propagates)."""
    B, h, w = a.shape
    return a.reshape(B, h // s, s, w // s, s).max((2, 4))


class JpegOracle:
    """Everything the comparison needs from the oracle alone for one input (x (B,3,H,W) float32, quality a number or
    (B,)): the fp64 output, the per-sample window, the undecided coefficients and their census per macroblock."""

    def __init__(self, x, quality):
        self.x = np.asarray(x, np.float32)
        self.quality = quality if np.ndim(quality) == 0 else np.asarray(quality, np.float32)
        self.B, _, self.H, self.W = self.x.shape
        self.ref, q64 = dp.diffjpeg(self.x, self.quality, return_quotients=True)
        _, q32 = dp.diffjpeg(self.x, self.quality, return_quotients=True, dtype=np.float32)
        self.deviation = np.max([np.abs(a.astype(np.float64) - b).reshape(self.B, -1).max(1) for a, b in zip(q32, q64)], 0)
        self.window = np.maximum(MIN_WINDOW, WINDOW_MARGIN * self.deviation)                      # (B,)
        self.quot_max = np.max([np.abs(b).reshape(self.B, -1).max(1) for b in q64], 0)
        self.undecided = [np.abs(q - np.floor(q) - 0.5) < self.window[:, None, None] for q in q64]
        self.Hp, self.Wp = q64[0].shape[1:]
        # undecided coefficients per macroblock: 16 x 16 of the luma plane, 8 x 8 of Cb and of Cr
        self.count = sum(u.reshape(self.B, self.Hp // 16, s, self.Wp // 16, s).sum((2, 4))
                         for u, s in zip(self.undecided, (16, 8, 8)))
        self.n_macroblocks = int(self.count.size)
        self.n_undecided_mb = int((self.count > 0).sum())
        self.max_undecided = int(self.count.max())
        self.over_cap = int((self.count > CAP).sum())

    def census(self):
        return dict(macroblocks=self.n_macroblocks, undecided_mb=self.n_undecided_mb, max_undecided=self.max_undecided,
                    over_cap=self.over_cap)

    def mb_error(self, out, ref=None):
        """(B, Hp/16, Wp/16): worst |out - ref| of each macroblock over the three channels, inside H x W."""
        d = np.abs(np.asarray(out, np.float64) - (self.ref if ref is None else ref)).max(1)
        return _mb_max(np.pad(d, ((0, 0), (0, self.Hp - self.H), (0, self.Wp - self.W))), 16)

    def assignments(self, b, my, mx):
        """The oracle on macroblock (b, my, mx) alone under every assignment of its n undecided roundings:
        (2^n, 3, h, w) with h, w <= 16 the part inside the image; row 0 is the fp64 rounding."""
        n = int(self.count[b, my, mx])
        ys, xs = slice(16 * my, min(16 * my + 16, self.H)), slice(16 * mx, min(16 * mx + 16, self.W))
        und = [u[b, s * my:s * (my + 1), s * mx:s * (mx + 1)] for u, s in zip(self.undecided, (16, 8, 8))]
        where = [(k, i, j) for k, u in enumerate(und) for i, j in zip(*np.nonzero(u))]
        assert len(where) == n <= CAP
        flips = [np.zeros((1 << n,) + u.shape, bool) for u in und]
        for bit, (k, i, j) in enumerate(where):
            flips[k][:, i, j] = (np.arange(1 << n) >> bit) & 1
        tile = np.repeat(self.x[b:b + 1, :, ys, xs], 1 << n, 0)
        q = self.quality if np.ndim(self.quality) == 0 else np.full(1 << n, self.quality[b], np.float32)
        return dp.diffjpeg(tile, q, flips=flips)


def jpeg_match(out, x, quality, bound=BOUND, oracle=None):
    """Compare `out` (B,3,H,W) with the oracle on (x, quality) macroblock by macroblock, crediting only the undecided
    roundings (module docstring).  `oracle`: a JpegOracle of the same (x, quality), to share its work between calls.
    Returns the report, a dict:
      ok            every macroblock matched
      macroblocks   how many there are; all of them are compared
      undecided_mb  how many hold an undecided quotient;  max_undecided: the most in one macroblock
      flipped_mb    how many matched only under an assignment other than the fp64 rounding
      worst         the largest error of a macroblock under the assignment accepted for it (the best one if none matched;
                    inf for a macroblock holding a NaN)
      failed        [(b, my, mx, error)] of the macroblocks without a matching assignment
      window, deviation, quot_max   per sample: the window, max |quot32 - quot64| and max |quot64| of the oracle
    Raises ValueError for an input with a macroblock over the cap."""
    o = oracle if oracle is not None else JpegOracle(x, quality)
    if o.over_cap:
        raise ValueError(f"{o.over_cap} macroblock(s) hold more than {CAP} undecided quotients (max {o.max_undecided}): "
                         "not an input this comparison is for")
    out = np.asarray(out)
    assert out.shape == o.x.shape, (out.shape, o.x.shape)
    err = o.mb_error(out)
    err = np.where(np.isnan(err), np.inf, err)                 # (a NaN pixel matches nothing)
    flipped, failed = 0, []
    for b, my, mx in zip(*np.nonzero(err > bound)):
        best = err[b, my, mx]
        if o.count[b, my, mx] > 0:
            ys, xs = slice(16 * my, min(16 * my + 16, o.H)), slice(16 * mx, min(16 * mx + 16, o.W))
            e = np.abs(np.asarray(out[b:b + 1, :, ys, xs], np.float64) - o.assignments(b, my, mx)).max((1, 2, 3))
            best = np.where(np.isnan(e), np.inf, e).min()
        err[b, my, mx] = best
        if best <= bound:
            flipped += 1
        else:
            failed.append((int(b), int(my), int(mx), float(best)))
    return dict(ok=not failed, macroblocks=o.n_macroblocks, undecided_mb=o.n_undecided_mb, max_undecided=o.max_undecided,
                flipped_mb=flipped, worst=float(err.max()), failed=failed,
                window=o.window, deviation=o.deviation, quot_max=o.quot_max)


def report_line(kernel, case, r, bound=BOUND):
    """One `DPSWEEP` line (the format of tests/test_gpu_datapath.py) from a jpeg_match report."""
    return (f"DPSWEEP {kernel:14s} {case:44s} err {r['worst']:.3e}  bound {bound:.1e}  mb {r['macroblocks']} "
            f"undecided {r['undecided_mb']} (max {r['max_undecided']}) flipped {r['flipped_mb']} left out 0")
