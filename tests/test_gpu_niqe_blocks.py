"""The NIQE kernels (ssl_amd/csrc/ssg_niqe.hip) past the six blocks of the fixture, on the generated cases of
niqe_cases.py (tests/test_cpu_niqe_blocks.py asserts what each of them reaches): niqe_fit's flag loop on its second
trip and its count folded over more than one wave, the seven row lanes of the column means on their second trip, NaN
rows in the middle and at the end of the covariance's rows, NaN rows of five patterns, two / one / no good row, a
column without a finite entry; aggd_index ending at both ends of its table and on one-sided maps; a batch of four.

The kernels are compared with the fp64 restatement (niqe_reference.py) run on the GPU's own planes, by
niqe_reference.compare_planes / compare_features / compare_score: plane 1 exact, plane 2 within 255 * 2^-44, the NaN
pattern and every alpha equal, the other features within 1e-10 relative, |q2 - q2_restatement| <= 64 cond(Sigma) 2.2e-16
q2.  Every case runs once (module cache); each test prints its share of its bound (pytest -s)."""
import numpy as np
import pytest
import torch

import niqe_cases as C
import niqe_reference as N
import test_cpu_niqe as TC

pytestmark = pytest.mark.gpu

U8_HWC, U8_CHW, F32_PLANE = 1, 2, 3
_CACHE = {}


def _need():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def device_input(name):
    """A case as the C ABI takes it: (contiguous device tensor with a batch axis, kind, crop)."""
    img, order, crop = C.image(name)
    return torch.from_numpy(np.array(img)).cuda()[None], (F32_PLANE if order == 'HW' else U8_HWC), crop


def all_of(t, kind, crop):
    """(scores, features, plane 1, plane 2) of a device batch."""
    from ssl_amd import metrics as M
    return (M._niqe_run(t, kind, crop, 'y', TC.PARAMS), M.niqe_features(t, kind, crop), *M.niqe_planes(t, kind, crop))


def run(name):
    """GPU planes, features and score of a case, and the restatement run on the GPU's own planes (once per case: the
    258 blocks of `trips` cost the restatement about 2 s)."""
    if name not in _CACHE:
        score, feat, p1, p2 = all_of(*device_input(name))
        torch.cuda.synchronize()
        p1, p2 = p1[0].cpu().numpy(), p2[0].cpu().numpy()
        rf, rt = N.features_from_planes(p1.astype(np.float64), p2)
        P = TC.params()
        _CACHE[name] = dict(p1=p1, p2=p2, feat=feat[0].cpu().numpy(), score=float(score[0]), rfeat=rf, rt=rt,
                            rfit=N.fit(rf, P["mu_pris_param"], P["cov_pris_param"]))
    return _CACHE[name]


@pytest.mark.parametrize("name", C.CASES)
def test_planes(name):
    _need()
    img, order, crop = C.image(name)
    r = run(name)
    nbh, nbw = C.BLOCKS[name]
    assert r["p1"].shape == (nbh * C.BS, nbw * C.BS)
    share = N.compare_planes(r["p1"], r["p2"], N.plane1(img, crop, order))
    print(f"{name} plane 2: {share:.3e} of the bound {N.PLANE2_BOUND:.3e}")


@pytest.mark.parametrize("name", C.CASES)
def test_features(name):
    """(the two cases without a score included: their rows still match, NaN entries and all)"""
    _need()
    r = run(name)
    assert r["feat"].shape[0] == C.BLOCKS[name][0] * C.BLOCKS[name][1]
    share = N.compare_features(r["feat"], r["rfeat"], r["rt"])
    nan = np.isnan(r["feat"])
    print(f"{name} features: {share:.3e} of the bound {N.FEATURE_BOUND:.0e}; {int(nan.any(1).sum())} rows with a NaN, "
          f"{int(nan.all(0).sum())} columns without a finite entry, min midpoint margin "
          f"{N.midpoint_margin(r['rt']).min():.3e}")


@pytest.mark.parametrize("name", C.CASES)
def test_score(name):
    _need()
    r = run(name)
    assert np.isnan(r["rfit"]["score"]) == (name in C.NAN_SCORE)     # the restatement on the GPU's planes, as on its own
    share = N.compare_score(r["score"], r["rfit"])
    if name in C.NAN_SCORE:
        assert np.isnan(r["score"])
        print(f"{name} score: NaN on both sides")
        return
    print(f"{name} score {r['score']:.9f}: |q2 - q2_restatement| / q2 = "
          f"{abs(r['score'] ** 2 - r['rfit']['q2']) / r['rfit']['q2']:.3e}, {share:.3e} of the bound "
          f"(cond {r['rfit']['cond']:.3e})")


def test_trips_fit_alone():
    """niqe_fit by itself at 258 rows: the restatement's fit of the GPU's OWN feature rows against the GPU's score, so
    that a failure of test_score[trips] can be told from one of niqe_features."""
    _need()
    r = run("trips")
    P = TC.params()
    assert r["feat"].shape[0] > C.NT + 1
    own = N.fit(r["feat"], P["mu_pris_param"], P["cov_pris_param"])
    share = N.compare_score(r["score"], own)
    print(f"trips, fit alone: {share:.3e} of the bound (cond {own['cond']:.3e})")


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _batch():
    return torch.from_numpy(np.stack([C.image(n)[0] for n in C.BATCH])).cuda()


def test_batch_of_four_equals_single_calls_and_repeats_bit_for_bit():
    """`patterns`, a natural plane, one with a black block and iid-uniform noise on blockIdx.y = 0 .. 3."""
    _need()
    batch = _batch()
    whole, again = all_of(batch, F32_PLANE, 0), all_of(batch, F32_PLANE, 0)
    singles = [all_of(batch[k:k + 1].contiguous(), F32_PLANE, 0) for k in range(len(C.BATCH))]
    torch.cuda.synchronize()
    assert whole[0].shape == (4,) and whole[1].shape == (4, 21, N.NF)
    for a, b in zip(whole, again):
        assert torch.equal(_bits(a), _bits(b))
    for k in range(len(C.BATCH)):
        for a, b in zip(whole, singles[k]):
            assert torch.equal(_bits(a[k:k + 1]), _bits(b)), k
    scores = [float(v) for v in whole[0]]
    assert all(np.isfinite(scores)) and len(set(scores)) == 4
    assert [int(torch.isnan(whole[1][k]).any(1).sum()) for k in range(4)] == [5, 0, 1, 0]
    # and the first member is the `patterns` case that the tests above hold to the restatement
    r = run("patterns")
    assert scores[0] == r["score"] and np.array_equal(whole[1][0].cpu().numpy(), r["feat"], equal_nan=True)
    print("batch scores", " ".join(f"{s:.9f}" for s in scores))


def test_rgb_bytes_as_hwc_and_chw_reach_the_same_plane_and_score():
    _need()
    img, order, crop = C.image("rgb")
    chw = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).cuda()[None]
    score, feat, p1, p2 = all_of(chw, U8_CHW, crop)
    torch.cuda.synchronize()
    r = run("rgb")
    assert np.array_equal(p1[0].cpu().numpy(), r["p1"]) and np.array_equal(p2[0].cpu().numpy(), r["p2"])
    assert np.array_equal(feat[0].cpu().numpy(), r["feat"])
    assert float(score[0]) == r["score"] and np.isfinite(r["score"])


POISON_CASES = ("waves", "patterns", "two_good")


def poison_cases():
    """What test_gpu_niqe_blocks_poison.py runs on the product build and again on the poisoned profiling build."""
    out = []
    for name in POISON_CASES:
        out += list(all_of(*device_input(name)))
    torch.cuda.synchronize()
    return out
