"""The generated NIQE cases (niqe_cases.py) on the restatement alone, no GPU output in any of it: that each case
reaches the loop, the table end or the NaN pattern it was made for (so that a later change of a seed or of a kernel
constant cannot hollow it out quietly), that no fit lies near a midpoint of the r(gam) table (what the GPU test's exact
alpha comparison rests on), that two orders of summation of the fit agree within the score's bound at up to 258 rows,
and that the comparisons the GPU test is made of (niqe_reference.compare_*) refuse wrong fits."""
import math

import numpy as np
import pytest

import niqe_cases as C
import niqe_reference as N
import test_cpu_niqe as TC

EVERY = C.CASES + C.BATCH[1:]
NAN_ROWS = dict(lanes=[], waves=sorted(C.WAVES_BLACK), trips=sorted(C.TRIPS_BLACK), patterns=[0, 6, 12, 18, 20],
                two_good=[2, 3, 4, 5, 6, 7], one_good=[1, 2, 3, 4, 5, 6, 7], dead_column=[0, 1], rgb=[],
                batch_natural=[], batch_black=[10], batch_uniform=[])


def R(name):
    return C.restated(name, TC.params())


def nan_rows(name):
    return np.flatnonzero(np.isnan(R(name)["feat"]).any(1)).tolist()


# ------------------------------------------------------------------------------------- what every case reaches ---
def test_shapes_follow_the_kernels_constants():
    """The block counts, and that they cross the thresholds they are named for."""
    for name in C.CASES:
        nbh, nbw = C.BLOCKS[name]
        img, order, crop = C.image(name)
        assert ((img.shape[0] - 2 * crop) // C.BS, (img.shape[1] - 2 * crop) // C.BS) == (nbh, nbw), name
        assert R(name)["feat"].shape == (nbh * nbw, N.NF), name
    assert (C.NT, C.FL) == (256, 7)              # the kernels' constants today; the three lines below hold for any
    nblk = {k: v[0] * v[1] for k, v in C.BLOCKS.items()}
    assert (nblk["lanes"], nblk["waves"], nblk["trips"], nblk["patterns"], nblk["rgb"]) == (8, 70, 258, 21, 10)
    assert nblk["lanes"] > C.FL                  # lane 0 makes a second trip, so lane FL - 1 has a row
    assert C.WAVE <= C.WAVES_BLACK[1] < nblk["waves"] <= 2 * C.WAVE and C.WAVES_BLACK[0] < C.WAVE
    assert nblk["trips"] > C.NT + 1 and nblk["trips"] - C.TRIPS_NBH <= C.NT + 1      # the smallest such 3-row plane
    assert C.TRIPS_BLACK[0] < C.NT and C.TRIPS_BLACK[1] == C.NT + 1
    assert C.image("rgb")[0].shape == (200, 492, 3) and C.image("rgb")[0].dtype == np.uint8
    assert all(C.image(n)[0].dtype == np.float32 and C.image(n)[1] == 'HW' for n in C.PLANE_CASES + C.BATCH)
    assert {C.image(n)[0].shape for n in C.BATCH} == {(288, 672)}


@pytest.mark.parametrize("name", EVERY)
def test_rows_with_a_nan(name):
    assert nan_rows(name) == NAN_ROWS[name]


def test_black_rows_sit_in_wave_1_and_in_the_second_trip():
    """`waves`: one NaN row among the flags wave 0 counts, one among wave 1's, good rows in both.  `trips`: row NT (good)
    and row NT + 1 (a NaN) belong to the flag loop's second trip, and the covariance skips a row in its middle."""
    w, t = nan_rows("waves"), nan_rows("trips")
    assert [r // C.WAVE for r in w] == [0, 1]
    assert [r // C.NT for r in t] == [0, 1] and C.NT not in t and 0 < t[0] < C.NT - 1
    assert R("trips")["feat"].shape[0] - len(t) == C.NT


def test_patterns_hold_distinct_nan_patterns_and_both_table_ends():
    feat, t = R("patterns")["feat"], R("patterns")["t"]
    nan = np.isnan(feat)
    rows = np.flatnonzero(nan.any(1))
    pats = {tuple(nan[r]) for r in rows}
    print(f"patterns: {len(rows)} rows with a NaN in {len(pats)} distinct patterns, {feat.shape[0] - len(rows)} good rows")
    assert len(pats) >= 4
    # one-sided maps: beta_l alone NaN and beta_r alone NaN, on both scales (columns o + 2, o + 3 of a shifted map)
    bl = [2 + 4 * k + 2 + 18 * s for s in (0, 1) for k in range(4)]
    only_l = nan[:, bl] & ~nan[:, [c + 1 for c in bl]]
    only_r = ~nan[:, bl] & nan[:, [c + 1 for c in bl]]
    for side in (only_l, only_r):
        assert side[:, :4].any() and side[:, 4:].any()
    # a NaN row that is not the black block's pattern (alpha finite, all else NaN), the only one the fixture has
    black = tuple(c not in N.ALPHA for c in range(N.NF))
    assert black in pats and len(pats - {black}) >= 3
    # both ends of the table, in rows that enter the covariance (so index 0 and the last index reach the score)
    r = N.table()[1]
    good = ~nan.any(1)
    tg = t[good]
    print(f"patterns: {(tg < r[0]).sum()} fits of good rows below r(gam)[0] = {r[0]:.4f} (smallest t {np.nanmin(t):.3e}), "
          f"{(tg > r[-1]).sum()} above r(gam)[-1] = {r[-1]:.4f} (largest t {np.nanmax(t):.6f})")
    assert (tg < r[0]).any() and (tg > r[-1]).any()
    a = feat[good][:, N.ALPHA]
    assert (a == N.GAM[0]).any() and (a == N.GAM[-1]).any()


def test_uniform_noise_lands_on_the_last_table_entry():
    """iid-uniform content (the batch's fourth member, and the fixture's c1) has t above the last r(gam) entry."""
    r = N.table()[1]
    t = R("batch_uniform")["t"]
    assert (t > r[-1]).any()
    assert (R("batch_uniform")["feat"][:, N.ALPHA][t > r[-1]] == N.GAM[-1]).all()


def test_good_row_counts_and_nan_scores():
    assert R("two_good")["feat"].shape[0] - len(nan_rows("two_good")) == 2
    assert R("one_good")["feat"].shape[0] - len(nan_rows("one_good")) == 1
    dead = np.isnan(R("dead_column")["feat"]).all(0)
    assert dead.any() and not dead.all()             # columns without a finite entry beside columns with some
    for name in EVERY:
        r = R(name)
        assert np.isnan(r["score"]) == (name in C.NAN_SCORE), name
        if name not in C.NAN_SCORE:
            assert r["ratio"] > 1e-12, (name, r["ratio"])
    assert len({R(n)["score"] for n in C.BATCH}) == 4


@pytest.mark.parametrize("name", EVERY)
def test_no_fit_within_1e9_of_a_midpoint(name):
    m = float(N.midpoint_margin(R(name)["t"]).min())
    print(f"{name}: smallest midpoint margin {m:.3e}")
    assert m > 1e-9


def test_flat_parts_are_level_zero_on_both_planes():
    """(niqe_cases.py's header: a flat non-zero level tests libm, not the kernel.)  Every 7 x 7 neighbourhood of one
    value, on plane 1 and on plane 2 of every case, holds 0."""
    for name in EVERY:
        for p in (R(name)["plane1"], R(name)["plane2"]):
            H, W = p.shape
            lo, hi = p.copy(), p.copy()
            pad = np.pad(p, 3, mode='edge')
            for i in range(7):
                for j in range(7):
                    v = pad[i:i + H, j:j + W]
                    lo, hi = np.minimum(lo, v), np.maximum(hi, v)
            assert not ((lo == hi) & (p != 0)).any(), name


@pytest.mark.parametrize("name", [n for n in EVERY if n != "trips"])       # (`trips` is `waves`' content, four times)
def test_no_feature_hangs_on_the_last_bit_of_the_window(name, monkeypatch):
    """The kernel's host code forms the 49 weights with the C library's exp and a running sum, the restatement with
    numpy's; they may differ in every last bit.  A case is a statement about the kernel only if that cannot move its
    features: with every weight one ulp up, and one ulp down (the sum of the weights passes 1 in one of the two), the
    restatement keeps its NaN pattern and every alpha, and the rest moves by less than a tenth of the feature bound.
    (Flat non-zero levels, two-level 1-pixel patterns seen at scale 2 and linear ramps all fail this: there I - mu is the
    rounding noise of mu.)"""
    r = R(name)
    w = N.window()
    worst = 0.0
    for toward in (np.inf, -np.inf):
        monkeypatch.setattr(N, "window", lambda: np.nextafter(w, toward))
        assert (N.window().sum() > 1) == (toward > 0)
        feat, _ = N.features_from_planes(r["plane1"], r["plane2"])
        monkeypatch.undo()
        assert np.array_equal(np.isnan(feat), np.isnan(r["feat"])), name
        assert np.array_equal(feat[:, N.ALPHA], r["feat"][:, N.ALPHA]), name
        a, b = feat[:, N.OTHER], r["feat"][:, N.OTHER]
        ok = ~np.isnan(b)
        worst = max(worst, float((np.abs(a - b)[ok] / np.abs(b[ok])).max()))
    print(f"{name}: features move by {worst:.3e} (relative) under one ulp of every weight")
    assert worst <= 0.1 * N.FEATURE_BOUND


# ------------------------------------------------------------------------------------ two orders of summation ---
def test_fit_in_two_orders_of_summation():
    """niqe_reference.fit (plain sums in row order, LU solve) against np.nanmean / np.cov / np.linalg.pinv (pairwise
    sums, SVD) on every case with a score, within the score's bound."""
    P = TC.params()
    worst = 0.0
    for name in EVERY:
        r = R(name)
        if name in C.NAN_SCORE:
            with np.errstate(all='ignore'):
                assert np.isnan(r["q2"])
            continue
        q2 = N.fit_by_numpy(r["feat"], P["mu_pris_param"], P["cov_pris_param"])
        share = abs(q2 - r["q2"]) / N.score_bound(r)
        print(f"{name}: {r['feat'].shape[0]} rows, |q2 - q2'| / q2 = {abs(q2 - r['q2']) / r['q2']:.3e}, "
              f"{share:.3e} of the bound")
        assert share <= 1.0, name
        worst = max(worst, share)
    # the bound has no row-count term; it would need one if the two orders used a noticeable part of it at 258 rows
    assert worst <= 0.01


# -------------------------------------------------------------------------- the comparisons refuse wrong fits ---
def fit_with(feat, good=None, ngood=None, mean_by_ngood=False, mean_rows=None):
    """niqe_fit's arithmetic with its decisions open to doctoring: which rows the covariance sums (`good`), the count
    it divides by (`ngood`), the nanmean's divisor, the rows the nanmean sees."""
    P = TC.params()
    feat = np.asarray(feat, np.float64)
    nan = np.isnan(feat)
    good = ~nan.any(1) if good is None else good
    n = int(good.sum()) if ngood is None else ngood
    rows = slice(None) if mean_rows is None else mean_rows
    total = np.where(nan, 0.0, feat)[rows].sum(0)
    mean = total / (n if mean_by_ngood else (~nan)[rows].sum(0))
    c = feat[good] - feat[good].sum(0) / n
    sigma = (P["cov_pris_param"] + c.T @ c / (n - 1)) / 2
    d = P["mu_pris_param"].reshape(-1) - mean
    return math.sqrt(float(d @ np.linalg.solve(sigma, d)))


def refused(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


def test_comparisons_accept_the_restatement_itself():
    for name in EVERY:
        r = R(name)
        assert N.compare_features(r["feat"].copy(), r["feat"], r["t"]) == 0.0
        if name in C.NAN_SCORE:
            assert N.compare_score(float('nan'), r) == 0.0 and refused(N.compare_score, 1.0, r)
        else:
            assert N.compare_score(fit_with(r["feat"]), r) < 1e-3, name
            assert refused(N.compare_score, float('nan'), r)


def test_score_comparison_refuses_wrong_fits():
    """Row 257 of `trips` is a black block, outside the covariance already; so beside the fit that never sees row 257
    (its alpha entries leave the nanmean) the covariance also loses row 256, the good row of the second trip."""
    t, w, p = R("trips"), R("waves"), R("patterns")
    last = t["feat"].shape[0] - 1
    assert last == C.NT + 1
    doctored = {}
    doctored["fit without row 257"] = (fit_with(t["feat"][:last]), t)
    g = ~np.isnan(t["feat"]).any(1)
    assert g[last - 1]
    g[last - 1] = False
    doctored["covariance without row 256"] = (fit_with(t["feat"], good=g), t)
    for name, r in (("waves", w), ("trips", t)):
        n64 = int((~np.isnan(r["feat"]).any(1))[:C.WAVE].sum())
        doctored[f"ngood over rows 0 .. 63 only ({name})"] = (fit_with(r["feat"], ngood=n64), r)
    for name, r in (("patterns", p), ("waves", w), ("two_good", R("two_good"))):
        doctored[f"nanmean divided by ngood ({name})"] = (fit_with(r["feat"], mean_by_ngood=True), r)
    for what, (score, r) in doctored.items():
        print(f"{what}: score {score:.9f} against {r['score']:.9f}, {abs(score ** 2 - r['q2']) / N.score_bound(r):.3e} "
              f"of the bound")
        assert refused(N.compare_score, score, r), what


def test_feature_comparison_refuses_wrong_rows():
    # rows in row-major block order (the score cannot see this: it is a permutation of the rows)
    for name in ("patterns", "lanes", "trips"):
        r = R(name)
        nbh, nbw = C.BLOCKS[name]
        rowmajor = r["feat"].reshape(nbw, nbh, N.NF).transpose(1, 0, 2).reshape(-1, N.NF)
        assert refused(N.compare_features, rowmajor, r["feat"], r["t"]), name
    r = R("patterns")
    feat, t, rg = r["feat"], r["t"], N.table()[1]
    # alpha one grid step off at index 0 (a finite t below the table, not the NaN early return) and at the last index
    for end, step, mask in ((0, 1, t < rg[0]), (-1, -2, t > rg[-1])):
        rows, fits = np.nonzero(mask)
        assert rows.size
        col = N.ALPHA[fits[0]]
        assert feat[rows[0], col] == N.GAM[end]
        bad = feat.copy()
        bad[rows[0], col] = N.GAM[step]
        assert refused(N.compare_features, bad, feat, t), end
    # beta_l finite where it must be NaN beside a finite beta_r
    nan = np.isnan(feat)
    hits = [(i, c) for c in (4, 8, 12, 16, 22, 26, 30, 34) for i in range(feat.shape[0]) if nan[i, c] and not nan[i, c + 1]]
    assert hits
    bad = feat.copy()
    bad[hits[0]] = feat[hits[0][0], hits[0][1] + 1]
    assert refused(N.compare_features, bad, feat, t)
    # a value 2e-10 off, and a plane 2 one bound off
    bad = feat.copy()
    bad[1, 1] *= 1 + 2e-10
    assert refused(N.compare_features, bad, feat, t)
    p1 = C.image("lanes")[0]
    p2 = N.plane2(p1.astype(np.float64))
    assert N.compare_planes(p1, p2, p1) == 0.0
    off = p2.copy()
    off[5, 7] += 2 * N.PLANE2_BOUND
    assert refused(N.compare_planes, p1, off, p1)
    other = p1.copy()
    other[0, 0] += 1
    assert refused(N.compare_planes, other, N.plane2(other.astype(np.float64)), p1)
