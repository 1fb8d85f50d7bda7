"""The layer sets of the spectral-normalisation tests, as numpy data: tests/test_cpu_specnorm.py runs every case through
the restatement (tests/specnorm_reference.py) and shows that it stays inside its own bounds, tests/test_gpu_specnorm.py
holds the kernels to them.

The unit sizes are those of ssl_amd/csrc/ssg_specnorm.hip (the CPU test asserts that the library exports the same): a
unit of launch A is STRIP columns by ROWS_A rows, of launch B ROWS_B rows, of launch C and of the backward CHUNK
elements.  Every one occurs at one less, equal and one more."""
import numpy as np

STRIP, ROWS_A, ROWS_B, CHUNK = 256, 64, 16, 4096

SMALLEST = [(1, 1), (1, 5), (5, 1)]
EDGES = ([(3, STRIP + d) for d in (-1, 0, 1)] + [(ROWS_A + d, 7) for d in (-1, 0, 1)]
         + [(ROWS_B + d, 9) for d in (-1, 0, 1)] + [(1, CHUNK - 1), (64, CHUNK // 64), (17, 241)])
assert 17 * 241 == CHUNK + 1
TALL = [(2 * ROWS_A + 2, STRIP + 44)]          # three row blocks of A, nine of B, ten chunks
LINEAR = [(100, 8192)]                         # Discriminator_VGG_128_SN's first linear layer
MIXED_8 = [(12, 3, 4, 4), (24, 12, 4, 4), (48, 24, 4, 4), (24, 48, 3, 3), (12, 24, 3, 3), (6, 12, 3, 3), (6, 6, 3, 3),
           (6, 6, 3, 3)]                       # UNetDiscriminatorSN's eight layers at num_feat = 6 (conv weights, 4-d)
MIXED_17 = SMALLEST + EDGES[:6] + MIXED_8[:5] + [(33, 65), (2, 1025), (70, 3)]
assert len(MIXED_17) == 17

CONTENTS = ("random", "zero", "rank1", "tiny", "orthogonal", "spike")


def rows_cols(shape):
    return shape[0], int(np.prod(shape[1:], dtype=np.int64))


def layer(shape, content, rng):
    """(W, u, v) fp32 of one layer: W of `shape`, u and v unit vectors as torch's initialisation leaves them."""
    R, K = rows_cols(shape)
    W = rng.standard_normal((R, K))
    u, v = rng.standard_normal(R), rng.standard_normal(K)
    if content == "zero":
        W = np.zeros((R, K))
    elif content == "rank1":               # W = 3 a b^T with unit a, b: the singular pair is (a, b), sigma = 3
        a, b = rng.standard_normal(R), rng.standard_normal(K)
        W = 3.0 * np.outer(a / np.linalg.norm(a), b / np.linalg.norm(b))
    elif content == "tiny":                # |t| and |s| fall below eps: both are divided by eps
        W = W * 1e-20
    elif content == "orthogonal" and R >= 2:
        W = np.rint(W * 8)                  # small integers: W^T u below is EXACTLY 0 in any order of the sum
        W[1] = W[0]
        u = np.zeros(R)
        u[0], u[1] = 1.0, -1.0
    elif content == "spike":               # one element 1e6 times the rest
        W[R // 2, K // 3] = 1e6
    if content != "orthogonal" or R < 2:
        u = u / max(np.linalg.norm(u), 1e-12)
    v = v / max(np.linalg.norm(v), 1e-12)
    return W.astype(np.float32).reshape(shape), u.astype(np.float32), v.astype(np.float32)


def layer_set(shapes, content="random", seed=0, nan_layer=None):
    """[(W, u, v)] for the shapes; nan_layer: that layer's W gets one NaN."""
    rng = np.random.default_rng(seed)
    out = [layer(s, content, rng) for s in shapes]
    if nan_layer is not None:
        W = out[nan_layer][0]
        W.reshape(-1)[W.size // 2] = np.nan
    return out


def gradients(shapes, seed=1):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s).astype(np.float32) for s in shapes]


# name -> (shapes, content, nan_layer): every case of the GPU test
CASES = {"smallest": (SMALLEST, "random", None), "edges": (EDGES, "random", None), "tall": (TALL, "random", None),
         "linear": (LINEAR, "random", None), "one": ([(33, 65)], "random", None), "eight": (MIXED_8, "random", None),
         "seventeen": (MIXED_17, "random", None), "nan_in_one": (MIXED_8, "random", 3)}
CASES.update({c: (SMALLEST + EDGES[:3] + EDGES[6:9] + MIXED_8[:2], c, None) for c in CONTENTS[1:]})
