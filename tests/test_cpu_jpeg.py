"""The JPEG sweep's test infrastructure, pinned on the CPU (no GPU needed): oracle/datapath_oracle.diffjpeg with its
`flips` / `dtype` arguments, the cases of tests/jpeg_cases.py and the branch-aware comparison of tests/jpeg_reference.py.

  - the oracle's default results are what they were before it had the two arguments;
  - no macroblock of any case holds more than jpeg_reference.CAP undecided quotients (on the oracle alone), so the
    comparison never leaves a macroblock out;
  - the reference's own fp32 output (fixture F25, tests/golden/make_golden_jpeg.py) passes the comparison on every case
    -- the reference stays inside the conditions, and the oracle is pinned at odd, 1-pixel and high-quality shapes;
  - outputs that are wrong in ways a kernel could be wrong are rejected.
Every comparison prints one `DPSWEEP` line (pytest -s).
"""
import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_reference as jr
from oracle import datapath_oracle as dp


def test_oracle_defaults_unchanged(golden):
    """Default arguments: bit-equal to the explicit defaults (no flip, float64) on F14, tensor and scalar quality, and
    equal to the float64 output recorded in F25 from the oracle as it was before it had the arguments (bit-equal where
    it was recorded; 2^-50 allows a numpy whose einsum sums in another order).  dtype=np.float32 returns float32."""
    g = golden("f14_diffjpeg")
    img = g["img"]
    for quality in (g["quality"], 50):
        out, quots = dp.diffjpeg(img, quality, return_quotients=True)
        out2, quots2 = dp.diffjpeg(img, quality, return_quotients=True, flips=[np.zeros(q.shape, bool) for q in quots],
                                   dtype=np.float64)
        assert out.dtype == np.float64 and np.array_equal(out, out2)
        assert all(np.array_equal(a, b) for a, b in zip(quots, quots2))
    rec = golden("f25_jpeg_sweep")["f14_scalar50_fp64"]
    assert rec.dtype == np.float64 and np.abs(dp.diffjpeg(img[:1], 50) - rec).max() <= 2.0 ** -50
    out32, quots32 = dp.diffjpeg(img, 50, return_quotients=True, dtype=np.float32)
    assert out32.dtype == np.float32 and all(q.dtype == np.float32 for q in quots32)
    assert np.abs(out32 - out).max() <= 1e-6       # (F14 holds no undecided quotient)


def test_flips_take_the_other_neighbour():
    """flips: a flipped coefficient is dequantised from floor + ceil - round, everything else is untouched -- on one
    macroblock, the luma DC and one Cr coefficient, checked through the linearity of the decoder before its clamp."""
    x, _ = jc.case("natural_33x31_q50")
    x = x[:1, :, :16, :16]
    base, quots = dp.diffjpeg(x, 50, return_quotients=True)
    flips = [np.zeros(q.shape, bool) for q in quots]
    flips[0][0, 8, 0] = True                      # DC of the lower-left luma block
    out = dp.diffjpeg(x, 50, flips=flips)
    d = (out - base) * 255
    q = quots[0][0, 8, 0]
    step = (np.floor(q) + np.ceil(q) - 2 * np.round(q)) * 16 / 8          # table 16, factor 1, DC gain 1/8
    assert np.abs(d[:, :, 8:, :8] - step).max() < 1e-9 and np.abs(d[:, :, :8]).max() == 0 and np.abs(d[:, :, :, 8:]).max() == 0
    flips = [np.zeros(q.shape, bool) for q in quots]
    flips[2][0, 0, 0] = True                      # Cr DC: R moves by 1.402 steps, B not at all, in all four luma blocks
    d = (dp.diffjpeg(x, 50, flips=flips) - base) * 255
    q = quots[2][0, 0, 0]
    step = (np.floor(q) + np.ceil(q) - 2 * np.round(q)) * 17 / 8
    assert np.abs(d[0, 0] - np.float64(np.float32(1.402)) * step).max() < 1e-9 and np.abs(d[0, 2]).max() < 1e-12


def test_cap_holds_on_every_case():
    """On the oracle alone: no macroblock over the cap, in any case; the flat grey cases at quality 50 have an
    undecided quotient in EVERY macroblock (what the whole-macroblock exclusion could not test at all)."""
    for tag in jc.TAGS:
        o = jc.oracle(tag)
        c = o.census()
        print(f"DPSWEEP jpeg census    {tag:28s} mb {c['macroblocks']:3d} undecided {c['undecided_mb']:3d} max {c['max_undecided']} "
              f"over cap {c['over_cap']}  fp32 deviation {o.deviation.max():.1e} window {o.window.max():.1e} |quot| {o.quot_max.max():.0f}")
        assert c["over_cap"] == 0 and c["max_undecided"] <= jr.CAP, tag
        assert np.all(o.window >= jr.MIN_WINDOW) and np.all(o.window >= 4 * o.deviation)
    for tag in ("grey_mb_32x48_q50", "grey_8x8_16x16_q50"):
        c = jc.oracle(tag).census()
        assert c["undecided_mb"] == c["macroblocks"] and c["max_undecided"] == 4, tag
    assert max(jc.oracle(t).window.max() for t in jc.TAGS) > 10 * jr.MIN_WINDOW      # quality 99 widens it


def test_cases_cover_what_they_claim():
    shapes = {jc.case(t)[0].shape[2:] for t in jc.TAGS}
    assert shapes == {(1, 1), (15, 17), (16, 16), (17, 15), (33, 31), (32, 48), (45, 83)}
    scalars = [jc.case(t)[1] for t in jc.TAGS if np.ndim(jc.case(t)[1]) == 0]
    assert {50, 30, 72.5, 72.3, 95} == set(scalars) and any(isinstance(q, int) for q in scalars)
    assert float(np.float32(72.3)) != 72.3 and float(np.float32(72.5)) == 72.5
    assert max(np.prod(jc.case(t)[0].shape) for t in jc.TAGS) == 5 * 3 * 45 * 83
    for q in (jc.QA, jc.QB):
        assert len(set(q.tolist())) == len(q) and q.max() < 100
    # an undecided Cb quotient exists (the shared chroma choice is exercised)
    assert sum(int(jc.oracle(t).undecided[1].sum()) for t in jc.TAGS) > 0


@pytest.mark.parametrize("tag", jc.TAGS)
def test_reference_fp32_passes(golden, tag):
    """F25: the reference's own fp32 output passes the comparison, every macroblock compared."""
    g = golden("f25_jpeg_sweep")
    assert list(g["tags"]) == jc.TAGS
    x, quality = jc.case(tag)
    r = jr.jpeg_match(g["out_" + tag], x, quality, oracle=jc.oracle(tag))
    print(jr.report_line("jpeg ref fp32", tag, r))
    assert r["ok"] and r["worst"] <= jr.BOUND, (tag, r["failed"])
    assert r["worst"] <= 1e-6                     # (measured: 4.4e-7 at worst, quality 99)


def test_flat_grey_needs_the_other_rounding(golden):
    """The reason for the comparison: on flat grey at quality 50 the reference's fp32 output is 7.8e-3 from the fp64
    oracle as it stands and within 1e-7 of it once the undecided DC roundings may go either way."""
    tag = "grey_mb_32x48_q50"
    out = golden("f25_jpeg_sweep")["out_" + tag]
    o = jc.oracle(tag)
    r = jr.jpeg_match(out, *jc.case(tag), oracle=o)
    assert np.abs(out - o.ref).max() > 5e-3 and r["ok"] and r["flipped_mb"] > 0 and r["worst"] < 1e-7


# ------------------------------------------------------------------ wrong outputs are rejected ----
def _rejected(tag, wrong, where=None):
    x, quality = jc.case(tag)
    o = jc.oracle(tag)
    good = jr.jpeg_match(o.ref, x, quality, oracle=o)
    assert good["ok"] and good["worst"] == 0 and good["flipped_mb"] == 0
    r = jr.jpeg_match(wrong, x, quality, oracle=o)
    print(jr.report_line("jpeg mutant", tag, r), "REJECTED" if not r["ok"] else "accepted", r["failed"][:2])
    assert not r["ok"] and r["worst"] > jr.BOUND
    if where is not None:
        assert {f[:3] for f in r["failed"]} == set(where)
    return r


def test_rejects_a_decided_coefficient_rounded_the_other_way():
    """One decided coefficient takes the other neighbour and only its macroblock fails: a luma AC coefficient of a
    natural image, and the Cb DC of a flat grey macroblock, where four undecided luma quotients are there to choose from."""
    for tag, k, (b, i, j) in (("natural_45x83_QA", 0, (2, 17, 34)), ("grey_mb_32x48_q50", 1, (1, 8, 16))):
        o = jc.oracle(tag)
        s = 16 if k == 0 else 8
        assert not o.undecided[k][b, i, j] and (k == 0 or o.count[b, i // s, j // s] == 4)
        flips = [np.zeros(u.shape, bool) for u in o.undecided]
        flips[k][b, i, j] = True
        _rejected(tag, dp.diffjpeg(*jc.case(tag), flips=flips), [(b, i // s, j // s)])


def test_rejects_a_transposed_luma_table_entry(monkeypatch):
    """Luma table entries (0, 1) = 12 and (1, 0) = 11 swapped."""
    tag = "natural_33x31_q72.5"
    jc.oracle(tag)                                # (built with the right table)
    swapped = dp._JPEG_Y.copy()
    swapped[0, 1], swapped[1, 0] = dp._JPEG_Y[1, 0], dp._JPEG_Y[0, 1]
    assert not np.array_equal(swapped, dp._JPEG_Y)
    with monkeypatch.context() as m:
        m.setattr(dp, "_JPEG_Y", swapped)
        wrong = dp.diffjpeg(*jc.case(tag))
    _rejected(tag, wrong)


def test_rejects_zero_chroma_in_the_padding():
    """Odd sides: the 2 x 2 chroma average of the last row / column takes a padded pixel, whose Cb and Cr are 128.  A
    kernel that takes them as 0 is the oracle run on the image padded by hand with the colour whose YCbCr is (0, 0, 0)."""
    tag = "natural_33x31_q50"
    x, quality = jc.case(tag)
    M1 = np.array([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]], np.float32).astype(np.float64)
    colour = np.linalg.solve(M1, np.array([0.0, -128.0, -128.0])) / 255
    padded = np.empty(x.shape[:2] + (48, 32), np.float64)
    padded[:] = colour[None, :, None, None]
    padded[:, :, :33, :31] = x
    wrong = dp.diffjpeg(padded, quality)[:, :, :33, :31]
    o = jc.oracle(tag)
    # only the macroblocks holding the last row (32) or the last column (30) can differ
    r = _rejected(tag, wrong)
    assert all(my == 2 or mx == 1 for _, my, mx, _ in r["failed"]) and len(r["failed"]) >= 4
    assert np.abs(wrong - o.ref)[:, :, :32, :16].max() < 1e-12


def test_rejects_inconsistent_chroma_choices():
    """A macroblock with an undecided Cb quotient: both choices are accepted, each for the whole macroblock; an output
    whose upper-left luma block follows one choice and the rest the other is rejected, although each 8 x 8 block alone
    agrees with an accepted output."""
    tag = "saturated_33x31_q50"
    x, quality = jc.case(tag)
    o = jc.oracle(tag)
    b, i, j = (int(v[0]) for v in np.nonzero(o.undecided[1]))
    my, mx = i // 8, j // 8
    assert o.count[b, my, mx] == 1 and 16 * my + 16 <= 33 and 16 * mx + 16 <= 31
    flips = [np.zeros(u.shape, bool) for u in o.undecided]
    flips[1][b, i, j] = True
    other = dp.diffjpeg(x, quality, flips=flips)
    for out in (o.ref, other):
        r = jr.jpeg_match(out, x, quality, oracle=o)
        assert r["ok"] and r["worst"] < 1e-12
    assert jr.jpeg_match(other, x, quality, oracle=o)["flipped_mb"] == 1
    ys, xs = slice(16 * my, 16 * my + 8), slice(16 * mx, 16 * mx + 8)
    assert np.abs(other - o.ref)[b, :, ys, xs].max() > 100 * jr.BOUND
    assert np.abs(other - o.ref)[b, :, 16 * my + 8:16 * my + 16, 16 * mx + 8:16 * mx + 16].max() > 100 * jr.BOUND
    mixed = o.ref.copy()
    mixed[b, :, ys, xs] = other[b, :, ys, xs]
    _rejected(tag, mixed, [(b, my, mx)])


def test_rejects_the_neighbouring_samples_quality():
    for tag in ("random2_15x17_QA", "natural_33x31_QB"):
        x, quality = jc.case(tag)
        r = _rejected(tag, dp.diffjpeg(x, np.roll(quality, 1)))
        assert {f[0] for f in r["failed"]} == set(range(len(quality)))


def test_rejects_nan_and_refuses_an_input_over_the_cap():
    tag = "grey_mb_32x48_q50"
    o = jc.oracle(tag)
    wrong = o.ref.copy()
    wrong[1, 2, 20, 40] = np.nan
    _rejected(tag, wrong, [(1, 1, 2)])
    # quality 99.99 on full-range noise: quotients beyond 300,000, a window of 0.1 and dozens of undecided quotients in
    # every macroblock -- not an input the comparison is for, and it says so instead of leaving macroblocks out
    rng = np.random.default_rng(3)
    x = (np.rint(rng.random((1, 3, 32, 32)) * 255) / 255).astype(np.float32)
    over = jr.JpegOracle(x, 99.99)
    assert over.over_cap == over.n_macroblocks == 4
    with pytest.raises(ValueError):
        jr.jpeg_match(over.ref, x, 99.99, oracle=over)
