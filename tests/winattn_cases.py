"""The window-attention cases shared by the CPU and GPU tests: the smallest shapes at which each thing can go wrong.

  one_window      1 x 8 x 8, 1 head of 1 channel, no shift: one unit, no mask, the shortest chain
  labels_s4/1/7   1 x 16 x 24, 2 heads of 30, shifts 4, 1, 7: all nine mask labels, both wrap directions, not square,
                  head_dim no multiple of 4 (a head's slice starts at an 8-byte boundary only)
  row_s4          1 x 8 x 16, 1 head of 5, shift 4: one window row, ys >= H - 8 holds for every row
  batch_d10/31/32 3 x 16 x 16, 6 heads, head_dim 10, 31 and the largest, shifts 3, 0 and 5
  second_trip     3 x 64 x 64, 6 heads of 10, shift 4: 1,152 (image, window, head) units on a grid capped at 1,020
                  workgroups (1,024 rounded down to a multiple of 6 heads): 132 workgroups take a second unit
and on 1 x 16 x 24, 2 heads of 30, the contents that the random ones do not reach:
  big_s4          scores of about +-80: one-hot rows, exp underflows, a masked entry at -100 comparable with an
                  unmasked one
  same_keys       identical keys, a zero table, no shift: P is uniform
  zeros_s4        all-zero qkv
  nan_s4          one NaN token
  one_window_dout a dout that is zero outside one window
The table has standard deviation 1 and is not symmetric under i <-> j (a transposed index shows).
"""
import numpy as np

TRAINING = dict(B=4, H=64, W=64, heads=6, d=30)        # the reference's training shape (tools/winattn_time.py)


def _case(name, B, H, W, heads, d, shift, content="random", seed=0):
    return dict(name=name, B=B, H=H, W=W, heads=heads, d=d, shift=shift, content=content, seed=seed)


SHAPES = [
    _case("one_window", 1, 8, 8, 1, 1, 0, seed=1),
    _case("labels_s4", 1, 16, 24, 2, 30, 4, seed=2),
    _case("labels_s1", 1, 16, 24, 2, 30, 1, seed=3),
    _case("labels_s7", 1, 16, 24, 2, 30, 7, seed=4),
    _case("row_s4", 1, 8, 16, 1, 5, 4, seed=5),
    _case("batch_d10", 3, 16, 16, 6, 10, 3, seed=6),
    _case("batch_d31", 3, 16, 16, 6, 31, 0, seed=7),
    _case("batch_d32", 3, 16, 16, 6, 32, 5, seed=8),
]
CONTENTS = [
    _case("big_s4", 1, 16, 24, 2, 30, 4, "big", seed=9),
    _case("same_keys", 1, 16, 24, 2, 30, 0, "same_keys", seed=10),
    _case("zeros_s4", 1, 16, 24, 2, 30, 4, "zeros", seed=11),
    _case("nan_s4", 1, 16, 24, 2, 30, 4, "nan", seed=12),
    _case("one_window_dout", 1, 16, 24, 2, 30, 4, "window_dout", seed=13),
]
SECOND_TRIP = _case("second_trip", 3, 64, 64, 6, 10, 4, seed=14)
SMALL = SHAPES + CONTENTS                    # every case the CPU tests walk
ALL = SMALL + [SECOND_TRIP]
NAN_TOKEN = (0, 5, 9)                        # (image, y, x) of the NaN token


def by_name(name):
    return next(c for c in ALL if c["name"] == name)


def make(case):
    """(qkv, table, dout, scale): fp32 arrays (B, H, W, 3 C), (225, heads), (B, H, W, C) and the module's d ** -0.5"""
    B, H, W, heads, d = (case[k] for k in ("B", "H", "W", "heads", "d"))
    C = heads * d
    rng = np.random.default_rng(1000 + case["seed"])
    qkv = rng.standard_normal((B, H, W, 3 * C)).astype(np.float32)
    table = rng.standard_normal((225, heads)).astype(np.float32)
    dout = rng.standard_normal((B, H, W, C)).astype(np.float32)
    content = case["content"]
    if content == "big":
        qkv[..., :2 * C] *= np.float32(6.3)          # scores of standard deviation 40
    elif content == "same_keys":
        qkv[..., C:2 * C] = qkv[0, 0, 0, C:2 * C]
        table[:] = 0
    elif content == "zeros":
        qkv[:] = 0
    elif content == "nan":
        qkv[NAN_TOKEN] = np.nan
    elif content == "window_dout":
        inside = np.zeros((H, W), dtype=bool)        # the pixels of the shifted window (1, 1)
        inside[np.ix_((np.arange(8, 16) + case["shift"]) % H, (np.arange(8, 16) + case["shift"]) % W)] = True
        dout[:, ~inside] = 0
    return qkv, table, dout, float(d) ** -0.5


_REFERENCE = {}


def reference(case):
    """The fp64 restatement's Result for a case, computed once and shared (do not modify it)."""
    import winattn_reference as R
    if case["name"] not in _REFERENCE:
        qkv, table, dout, scale = make(case)
        _REFERENCE[case["name"]] = R.evaluate(qkv, table, case["heads"], case["shift"], scale, dout)
    return _REFERENCE[case["name"]]
