"""What of the multi-tensor EMA update (ssl_amd/csrc/ssg_multi.hip, ssl_amd/ema.py) can be checked without a device:
the table the host builds, every refusal of the C ABI, the restatement tests/ema_reference.py against the reference's
recorded LitEma run (tests/golden/f34_ema.npz, written by make_golden_ema.py), and the Python classes on CPU tensors,
bit for bit."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch
from torch import nn

import ema_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f34_ema.npz")
WORD = 8


@pytest.fixture(scope="module")
def L():
    from ssl_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def fixture():
    with np.load(GOLDEN) as z:
        return {k: np.asarray(z[k]) for k in z.files}


def _arr(values):
    return np.ascontiguousarray(values, dtype=np.uintp)


def _fill(L, dst, src, counts):
    d, s, c = _arr(dst), _arr(src), _arr(counts)
    nbytes = L.ssg_multi_table_bytes(len(c), c.ctypes.data)
    table = np.zeros(nbytes // WORD, dtype=np.uint64)
    rc = L.ssg_multi_table_fill(len(c), d.ctypes.data, s.ctypes.data, c.ctypes.data, table.ctypes.data, nbytes)
    return rc, table


# ---- the C ABI ----
def test_symbols_have_the_headers_prototypes(L):
    from ssl_amd import _lib
    size_t, ptr = ctypes.c_size_t, ctypes.c_void_p
    want = {"ssg_multi_chunk": (ctypes.c_int, []), "ssg_multi_grid_cap": (ctypes.c_int, []),
            "ssg_multi_chunks": (size_t, [size_t, ptr]), "ssg_multi_table_bytes": (size_t, [size_t, ptr]),
            "ssg_multi_table_fill": (ctypes.c_int, [size_t, ptr, ptr, ptr, ptr, size_t]),
            "ssg_multi_apply": (ctypes.c_int, [ptr, size_t, ctypes.c_int, ctypes.c_float, ctypes.c_float, ptr, ptr])}
    for name, proto in want.items():
        assert _lib.PROTOTYPES[name] == proto, name
        assert getattr(L, name).argtypes == proto[1]
    assert [_lib.CONSTANTS["SSG_MT_" + k] for k in ("EMA", "LIT", "COPY")] == [R.EMA, R.LIT, R.COPY]
    assert L.ssg_abi_version() == 6
    assert L.ssg_multi_chunk() >= 4 and L.ssg_multi_chunk() % 4 == 0 and L.ssg_multi_grid_cap() >= 1


@pytest.mark.parametrize("residue", [0, 4, 8, 12])
def test_table_covers_every_element_once_in_order(L, residue):
    chunk = L.ssg_multi_chunk()
    counts = [0, 1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 5]
    dst = [0x100000 * (i + 1) + residue for i in range(len(counts))]
    src = [0x90000000 + 0x100000 * i + (residue + 4 * i) % 16 for i in range(len(counts))]
    rc, table = _fill(L, dst, src, counts)
    assert rc == 0
    n_chunks = sum(-(-n // chunk) for n in counts)
    assert L.ssg_multi_chunks(len(counts), _arr(counts).ctypes.data) == n_chunks
    assert table.size == 4 + 3 * len(counts) + n_chunks
    assert table[:4].tolist() == [len(counts), n_chunks, chunk, 0]
    records = table[4:4 + 3 * len(counts)].reshape(-1, 3)
    assert records.tolist() == [list(r) for r in zip(dst, src, counts)]
    words = table[4 + 3 * len(counts):]
    covered = []                                     # (tensor, first element, one past the last), chunk by chunk
    for w in words.tolist():
        t, k = w >> 32, w & 0xffffffff
        assert t < len(counts) and k * chunk < counts[t]
        covered.append((t, k * chunk, min(counts[t], (k + 1) * chunk)))
    want = [(t, o, min(n, o + chunk)) for t, n in enumerate(counts) for o in range(0, n, chunk)]
    assert covered == want                           # every element once, in tensor order and element order


def test_an_empty_set_is_a_header(L):
    rc, table = _fill(L, [], [], [])
    assert rc == 0 and table.tolist() == [0, 0, L.ssg_multi_chunk(), 0]
    rc, table = _fill(L, [0, 0], [0, 0], [0, 0])     # empty tensors: records, no chunk, pointers unused
    assert rc == 0 and table[:2].tolist() == [2, 0] and table.size == 4 + 6


def test_every_refusal_leaves_the_arguments_untouched(L):
    from ssl_amd import _lib
    C = _lib.CONSTANTS
    chunk = L.ssg_multi_chunk()
    d, s, c = _arr([0x1000, 0x2000]), _arr([0x3000, 0x4000]), _arr([5, 7])
    nbytes = L.ssg_multi_table_bytes(2, c.ctypes.data)
    assert nbytes == WORD * (4 + 6 + 2)
    table = np.full(nbytes // WORD + 1, 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    before = table.copy()
    fill = lambda d_, s_, c_, t_=table.ctypes.data, b_=nbytes, n_=2: L.ssg_multi_table_fill(  # noqa: E731
        n_, None if d_ is None else d_.ctypes.data, None if s_ is None else s_.ctypes.data,
        None if c_ is None else c_.ctypes.data, t_, b_)
    assert fill(d, s, c, t_=None) == C["SSG_E_BADARG"]
    assert fill(None, s, c) == fill(d, None, c) == fill(d, s, None) == C["SSG_E_BADARG"]
    assert fill(_arr([0, 0x2000]), s, c) == C["SSG_E_BADARG"]                 # a null address of a non-empty tensor
    for off in (1, 2, 3):
        assert fill(_arr([0x1000 + off, 0x2000]), s, c) == C["SSG_E_ALIGN"]
        assert fill(d, _arr([0x3000, 0x4000 + off]), c) == C["SSG_E_ALIGN"]
    assert fill(d, s, c, t_=table.ctypes.data + 4) == C["SSG_E_ALIGN"]
    assert fill(d, s, c, b_=nbytes - 1) == C["SSG_E_WORKSPACE"]
    huge = _arr([5, chunk << 31])                                               # 2^31 chunks: no int holds the count
    assert fill(d, s, huge) == C["SSG_E_TOOLARGE"]
    assert L.ssg_multi_table_bytes(2, huge.ctypes.data) == 0
    assert L.ssg_multi_chunks(2, huge.ctypes.data) == 2 ** 31
    assert np.array_equal(table, before)
    assert d.tolist() == [0x1000, 0x2000] and s.tolist() == [0x3000, 0x4000] and c.tolist() == [5, 7]
    assert fill(d, s, c) == 0 and table[-1] == before[-1] and table[1] == 2
    # ssg_multi_apply: every refusal is decided before the launch (no device is touched: the "table" is host memory)
    t, w = table.ctypes.data, np.zeros(2, dtype=np.float32)
    nan = float("nan")
    filled = table.copy()
    assert L.ssg_multi_apply(None, 2, R.EMA, 0.5, 0.5, None, None) == C["SSG_E_BADARG"]
    assert L.ssg_multi_apply(t, 2, -1, 0.5, 0.5, None, None) == L.ssg_multi_apply(t, 2, 3, 0.5, 0.5, None, None) \
        == C["SSG_E_BADARG"]
    assert L.ssg_multi_apply(t, 2, R.EMA, nan, 0.5, None, None) == L.ssg_multi_apply(t, 2, R.COPY, 0.5, nan, None, None) \
        == C["SSG_E_BADARG"]
    assert L.ssg_multi_apply(t, 2, R.LIT, 0.5, 0.5, None, None) == C["SSG_E_BADARG"]
    assert L.ssg_multi_apply(t + 4, 2, R.EMA, 0.5, 0.5, None, None) == C["SSG_E_ALIGN"]
    assert L.ssg_multi_apply(t, 2, R.LIT, 0.5, 0.5, w.ctypes.data + 2, None) == C["SSG_E_ALIGN"]
    assert L.ssg_multi_apply(t, 2 ** 31, R.EMA, 0.5, 0.5, None, None) == C["SSG_E_TOOLARGE"]
    assert L.ssg_multi_apply(t, 0, R.COPY, 0.0, 0.0, None, None) == 0         # nothing to launch
    assert np.array_equal(table, filled) and w.tolist() == [0.0, 0.0]


# ---- the restatement against the reference's recorded run ----
def _fixture_net(fixture):
    """The fixture's model and perturbations from the recorded values."""
    net = R.fixture_model({k[5:]: v for k, v in fixture.items() if k.startswith("init_")})
    pert = {n: torch.from_numpy(fixture["pert_" + n]) for n, _ in net.named_parameters()}
    assert all(v.shape[0] == R.FIXTURE_STEPS for v in pert.values())
    return net, pert


def test_fixture_holds_numbers_and_names_only_and_stays_small(fixture):
    assert os.path.getsize(GOLDEN) < 32 * 1024
    assert all(v.dtype in (np.float32, np.int32) or v.dtype.kind == "U" for v in fixture.values())
    assert fixture["keys"].tolist() == ["decay", "num_updates", "0weight", "1weight", "1bias"]    # 0.bias is frozen
    assert fixture["num_updates"].tolist() == list(range(1, 13)) and int(fixture["fixed_num_updates"]) == -1
    assert float(fixture["decay"]) == R.FIXTURE_DECAY


def test_restatement_equals_the_references_run_bit_for_bit(fixture):
    for prefix, steps, decay, counts in (("shadow_", R.FIXTURE_STEPS, R.FIXTURE_DECAY, True),
                                         ("fixed_shadow_", R.FIXED_STEPS, R.FIXED_DECAY, False)):
        net, pert = _fixture_net(fixture)
        names = {n: n.replace(".", "") for n, p in net.named_parameters() if p.requires_grad}
        shadow = {s: dict(net.named_parameters())[n].detach().clone() for n, s in names.items()}
        dec, num = torch.tensor(decay, dtype=torch.float32), torch.tensor(0 if counts else -1, dtype=torch.int)
        used = []
        for t in range(steps):
            R.perturb(net, pert, t)
            d, w = R.lit_scalars(dec, num)
            used.append(float(d))
            for n, s in names.items():
                R.lit_update(shadow[s], dict(net.named_parameters())[n].detach(), w)
                assert R.same_bits(shadow[s], torch.from_numpy(fixture[prefix + s][t])), (prefix, s, t)
        if counts:
            assert int(num) == steps
            want = [min(np.float32(decay), np.float32(1 + n) / np.float32(10 + n)) for n in range(1, steps + 1)]
            assert used == [float(v) for v in want] and used[7] == used[-1] == decay and used[6] < decay
        else:
            assert int(num) == -1 and used == [float(np.float32(decay))] * steps


# ---- the Python classes on CPU tensors ----
def _nets(seed=0, dtype=torch.float32):
    torch.manual_seed(seed)
    make = lambda: nn.Sequential(nn.Conv2d(3, 5, 3), nn.PReLU(), nn.Conv2d(5, 2, 1, bias=False), nn.Linear(7, 3))  # noqa: E731
    return make().to(dtype), make().to(dtype)


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.999, 0.9999, 1.0])
def test_model_ema_on_cpu_tensors_equals_the_expression(decay):
    from ssl_amd import ema
    net, avg = _nets()
    want = {k: p.detach().clone() for k, p in avg.named_parameters()}
    m = ema.ModelEma(net, avg)
    fn_net, fn_avg = copy.deepcopy(net), copy.deepcopy(avg)
    e_net, e_avg = copy.deepcopy(net), copy.deepcopy(avg)
    for _ in range(3):
        m.update(decay)
        ema.model_ema(fn_net, fn_avg, decay)
        ema.update_E(e_net, e_avg, decay)
        for k, p in net.named_parameters():
            R.ema_update(want[k], p.detach(), decay)
    for k, p in avg.named_parameters():
        assert R.same_bits(p, want[k]), k
        assert R.same_bits(dict(fn_avg.named_parameters())[k], want[k]) and R.same_bits(dict(e_avg.named_parameters())[k], want[k])
    assert m._ema.rebuilds == 1
    m.copy()
    for k, p in avg.named_parameters():
        assert R.same_bits(p, dict(net.named_parameters())[k])


def test_function_forms_keep_one_updater_per_pair_of_modules():
    from ssl_amd import ema
    net, avg = _nets()
    ema.model_ema(net, avg)
    first = ema._cached(net, avg, "ema")
    ema.model_ema(net, avg)
    assert ema._cached(net, avg, "ema") is first and first._ema.rebuilds == 1
    assert ema._cached(net, avg, "net") is not first
    n = len(ema._CACHE)
    del net, avg, first
    import gc
    gc.collect()
    assert len(ema._CACHE) == n - 1                  # the cache does not keep the modules alive


def test_wrapped_modules_are_unwrapped_and_a_missing_name_raises():
    from ssl_amd import ema
    net, avg = _nets()
    want = {k: R.ema_update(p.detach().clone(), dict(net.named_parameters())[k].detach(), 0.9)
            for k, p in avg.named_parameters()}
    ema.ModelEma(nn.DataParallel(net), avg).update(0.9)
    for k, p in avg.named_parameters():
        assert R.same_bits(p, want[k]), k
    assert ema.get_bare_model(nn.DataParallel(net)) is net and ema.get_bare_model(net) is net
    short = nn.Sequential(nn.Conv2d(3, 5, 3))
    with pytest.raises(KeyError):
        ema.ModelEma(short, avg)                     # model_ema walks the EMA network's names
    with pytest.raises(KeyError):
        ema.update_E(net, short)                     # update_E walks the generator's
    ema.ModelEma(net, short).update()                # the other way round every name is found


def test_fp64_and_mismatched_pairs_take_the_expression():
    from ssl_amd import ema
    net, avg = _nets(dtype=torch.float64)
    want = {k: R.ema_update(p.detach().clone(), dict(net.named_parameters())[k].detach(), 0.99)
            for k, p in avg.named_parameters()}
    m = ema.ModelEma(net, avg)
    m.update(0.99)
    for k, p in avg.named_parameters():
        assert p.dtype == torch.float64 and torch.equal(p.detach(), want[k]), k
    assert m._ema._tables == []


def test_rebuild_follows_new_storage():
    from ssl_amd import ema
    net, avg = _nets()
    m = ema.ModelEma(net, avg)
    m.update(0.9)
    p = net[0].weight
    p.data = p.data.clone() + 1.0
    want = R.ema_update(avg[0].weight.detach().clone(), p.detach(), 0.9)
    m.update(0.9)
    assert m._ema.rebuilds == 2 and R.same_bits(avg[0].weight, want)
    m.update(0.9)
    assert m._ema.rebuilds == 2


def _run_lit(fixture, cls_kwargs, prefix, steps):
    from ssl_amd import ema
    net, pert = _fixture_net(fixture)
    lit = ema.LitEma(net, **cls_kwargs)
    for t in range(steps):
        R.perturb(net, pert, t)
        lit(net)
        for s in lit.m_name2s_name.values():
            assert R.same_bits(dict(lit.named_buffers())[s], torch.from_numpy(fixture[prefix + s][t])), (s, t)
    return net, lit


def test_lit_ema_equals_the_references_run(fixture):
    net, lit = _run_lit(fixture, dict(decay=R.FIXTURE_DECAY), "shadow_", R.FIXTURE_STEPS)
    assert int(lit.num_updates) == int(fixture["num_updates"][-1]) and lit.num_updates.dtype == torch.int32
    assert list(lit.state_dict().keys()) == fixture["keys"].tolist()
    assert lit.m_name2s_name == {"0.weight": "0weight", "1.weight": "1weight", "1.bias": "1bias"}
    net, lit = _run_lit(fixture, dict(decay=R.FIXED_DECAY, use_num_upates=False), "fixed_shadow_", R.FIXED_STEPS)
    assert int(lit.num_updates) == -1
    with pytest.raises(ValueError):
        type(lit)(net, decay=1.5)


def test_lit_ema_state_dict_round_trip(fixture):
    from ssl_amd import ema
    half = R.FIXTURE_STEPS // 2
    net, lit = _run_lit(fixture, dict(decay=R.FIXTURE_DECAY), "shadow_", half)
    state = copy.deepcopy(lit.state_dict())
    other = ema.LitEma(R.fixture_model(), decay=0.9, use_num_upates=False)
    assert other._counting is False
    other.load_state_dict(state)
    assert other._counting is True and int(other.num_updates) == half and float(other.decay) == R.FIXTURE_DECAY
    twin = copy.deepcopy(lit)                           # a copy starts without the original's tables
    assert twin._forward.rebuilds == 0 and twin._forward._keep == [] and lit._forward.rebuilds == 1
    assert torch.equal(twin.state_dict()["0weight"], lit.state_dict()["0weight"])
    _, pert = _fixture_net(fixture)
    for t in range(half, R.FIXTURE_STEPS):              # the loaded copy goes on as the reference's run did
        R.perturb(net, pert, t)
        other(net)
        for s in other.m_name2s_name.values():
            assert R.same_bits(dict(other.named_buffers())[s], torch.from_numpy(fixture["shadow_" + s][t])), (s, t)


def test_lit_ema_store_copy_to_restore(fixture):
    net, lit = _run_lit(fixture, dict(decay=R.FIXTURE_DECAY), "shadow_", 3)
    live = {n: p.detach().clone() for n, p in net.named_parameters()}
    lit.store(net.parameters())
    assert all(not c.requires_grad and c.data_ptr() != p.data_ptr() for c, p in zip(lit.collected_params, net.parameters()))
    lit.copy_to(net)
    for n, p in net.named_parameters():
        if p.requires_grad:
            assert R.same_bits(p, torch.from_numpy(fixture["shadow_" + n.replace(".", "")][2])), n
        else:
            assert R.same_bits(p, live[n]), n           # the frozen parameter is not touched
    held = lit.collected_params
    lit.restore(net.parameters())
    for n, p in net.named_parameters():
        assert R.same_bits(p, live[n]), n
    lit.store(net.parameters())
    assert all(a is b for a, b in zip(held, lit.collected_params))     # the same buffers serve the next validation


@pytest.mark.parametrize("n_tensors", [3, 300])
def test_update_is_one_apply_whatever_the_number_of_tensors(monkeypatch, n_tensors):
    """The launch count, with the library call counted by a wrapper: CPU tensors are declared native and the table stays
    on the host, the counted apply does the arithmetic of the table it is handed, so the result is checked as well."""
    from ssl_amd import ema
    real = ema._lib.lib()
    calls = []

    class Counting:
        def __getattr__(self, name):
            return getattr(real, name)

        def ssg_multi_apply(self, table, n_chunks, kind, d, a, w, stream):
            calls.append((n_chunks, kind))
            words = np.ctypeslib.as_array(ctypes.cast(table, ctypes.POINTER(ctypes.c_uint64)), (4,))
            nt, nc = int(words[0]), int(words[1])
            words = np.ctypeslib.as_array(ctypes.cast(table, ctypes.POINTER(ctypes.c_uint64)), (4 + 3 * nt + nc,))
            assert nc == n_chunks
            for dst, src, n in words[4:4 + 3 * nt].reshape(-1, 3).tolist():
                e = np.ctypeslib.as_array(ctypes.cast(dst, ctypes.POINTER(ctypes.c_float)), (n,))
                p = np.ctypeslib.as_array(ctypes.cast(src, ctypes.POINTER(ctypes.c_float)), (n,))
                R.apply(kind, torch.from_numpy(e), torch.from_numpy(p), decay=d)
            return 0

    monkeypatch.setattr(ema, "_library", lambda: Counting())
    monkeypatch.setattr(ema, "_on_gpu", lambda t: True)
    monkeypatch.setattr(ema, "_upload", lambda host, device: host)
    gen = torch.Generator().manual_seed(n_tensors)
    net, avg = nn.Module(), nn.Module()
    for i in range(n_tensors):
        shape = (1 + i % 64,) if i % 3 else (2, 1 + i % 7, 3)
        net.register_parameter(f"p{i}", nn.Parameter(torch.randn(shape, generator=gen)))
        avg.register_parameter(f"p{i}", nn.Parameter(torch.randn(shape, generator=gen)))
    want = {k: R.ema_update(p.detach().clone(), dict(net.named_parameters())[k].detach(), 0.5)
            for k, p in avg.named_parameters()}
    m = ema.ModelEma(net, avg)
    m.update(0.5)                                  # 0.5 and 1 - 0.5 are exact in fp32: d == decay for the counted apply
    assert len(calls) == 1 and calls[0][1] == R.EMA and m._ema._fallback == []
    for k, p in avg.named_parameters():
        assert R.same_bits(p, want[k]), k
    m.update(0.5)
    m.copy()
    assert [c[1] for c in calls] == [R.EMA, R.EMA, R.COPY] and m._ema.rebuilds == 1
