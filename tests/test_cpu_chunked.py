"""What the two ragged one-launch families (ssg_multi.hip, ssg_mcrit.hip) share on the host, checked without a device:
the chunk count behind ssg_multi_chunks, ssg_multi_table_bytes and ssg_mcrit_workspace_bytes, and the "dense strides"
predicate behind ssl_amd.ema's native pairs and ssl_amd.engine.multi_pair_is_native.  Each side is held to a
restatement written out here, so the tests say the same of any two versions of the code."""
import numpy as np
import pytest
import torch

INT_MAX = 2 ** 31 - 1
WORD = 8


@pytest.fixture(scope="module")
def L():
    from ssl_amd import _lib
    return _lib.lib()


def _arr(values):
    return np.ascontiguousarray(values, dtype=np.uintp)


def _sizes(L, counts):
    """(ssg_multi_chunks, words of ssg_multi_table_bytes beyond header and records, doubles of ssg_mcrit_workspace_bytes)"""
    c, n = _arr(counts), len(counts)
    table = L.ssg_multi_table_bytes(n, c.ctypes.data)
    assert table % WORD == 0 and L.ssg_mcrit_workspace_bytes(n, c.ctypes.data) % 8 == 0
    return (L.ssg_multi_chunks(n, c.ctypes.data), table // WORD - (4 + 3 * n) if table else 0,
            L.ssg_mcrit_workspace_bytes(n, c.ctypes.data) // 8)


def test_the_three_chunk_counts_are_the_sum_of_the_ceilings(L):
    cm, cc = L.ssg_multi_chunk(), L.ssg_mcrit_chunk()
    edge = sorted({0, 1, cm - 1, cm, cm + 1, cc - 1, cc, cc + 1})
    for counts in [[n] for n in edge] + [edge, edge[::-1], [cm + 1] * 7 + [0, 1, cc + 1]]:
        multi, table, crit = _sizes(L, counts)
        assert multi == table == sum(-(-n // cm) for n in counts), counts
        assert crit == sum(-(-n // cc) for n in counts), counts


def test_a_count_that_no_int_holds_is_refused_by_each_in_its_own_way(L):
    cm, cc = L.ssg_multi_chunk(), L.ssg_mcrit_chunk()
    most = lambda chunk: [chunk * INT_MAX - (chunk - 1)]       # noqa: E731  INT_MAX chunks, the last of one element
    assert _sizes(L, most(cm))[:2] == (INT_MAX, INT_MAX) and _sizes(L, most(cc))[2] == INT_MAX
    for over in (lambda c: [c * INT_MAX + 1], lambda c: [c << 31], lambda c: [c << 30, 0, c << 30],
                 lambda c: [c * INT_MAX, 1]):
        assert _sizes(L, over(cm))[:2] == (INT_MAX + 1, 0), over(cm)
        assert _sizes(L, over(cc))[2] == 0, over(cc)


# ---- dense strides ----
def _by_arithmetic(t):
    """The EMA's restatement: over the dimensions of size != 1 in stride order, each stride is the product of the sizes
    below it."""
    expect = 1
    for stride, size in sorted((st, sz) for sz, st in zip(t.shape, t.stride()) if sz != 1):
        if stride != expect:
            return False
        expect *= size
    return True


def _by_permutation(t):
    """The criterion's restatement: permuted into descending stride order the tensor is contiguous."""
    return t.permute(sorted(range(t.dim()), key=lambda i: -t.stride(i))).is_contiguous()


def _layouts():
    x = torch.zeros(2, 3, 4, 5)
    yield "contiguous", x, True
    yield "channels_last", x.contiguous(memory_format=torch.channels_last), True
    yield "permuted", x.permute(2, 0, 3, 1), True
    yield "permuted channels_last", x.contiguous(memory_format=torch.channels_last).permute(3, 1, 0, 2), True
    for pos in range(4):
        shape = [2, 3, 4, 5]
        shape[pos] = 1
        y = torch.zeros(shape)
        yield f"size 1 at {pos}", y, True
        yield f"size 1 at {pos}, channels_last", y.contiguous(memory_format=torch.channels_last), True
        strides = list(y.stride())
        strides[pos] = 77                                             # a size-1 dimension's stride means nothing
        yield f"size 1 at {pos}, stride 77", y.as_strided(shape, strides), True
    yield "all of size 1", torch.zeros(1, 1, 1, 1), True
    yield "rows with a gap", x[:, 1:3], False
    yield "every other column", x[..., ::2], False
    yield "a gap behind a size 1", x[:, :, :1, :3], False
    yield "the leading slice", x[:1], True
    yield "expanded", torch.zeros(3, 1).expand(3, 4), False
    yield "expanded in front", torch.zeros(5).expand(2, 5), False
    yield "no element", torch.zeros(0), True
    yield "no row", torch.zeros(0, 3), True
    yield "one element", torch.zeros(1), True
    yield "one element, 0-d", torch.zeros(()), True
    yield "one element out of many", x[1:2, 2:3, 3:4, 4:5], True


@pytest.mark.parametrize("name,t,want", list(_layouts()), ids=[n for n, _, _ in _layouts()])
def test_dense_strides_is_both_restatements(name, t, want):
    from ssl_amd import ema
    assert _by_arithmetic(t) == want and _by_permutation(t) == want        # the two restatements agree on this layout
    assert ema._dense(t) is want


def test_where_the_restatements_part_the_ema_rule_holds():
    """A tensor without elements whose empty dimension is not the first: every such tensor "is contiguous" to torch, the
    arithmetic says no.  The criterion refuses empty tensors before it asks, so only the EMA meets these, and it keeps
    its answer: such a pair goes to torch's expression, which does nothing."""
    from ssl_amd import ema
    t = torch.zeros(2, 0, 3)
    assert _by_permutation(t) and not _by_arithmetic(t)
    assert ema._dense(t) is False
