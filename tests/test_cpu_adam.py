"""What of the one-launch Adam / AdamW step (ssl_amd/csrc/ssg_multi.hip, ssl_amd/optim.py) can be checked without a
device: the header's prototypes, the table and the gradient array the host builds, every refusal of the C ABI, the
restatement tests/adam_reference.py and torch's own CPU Adam against the fp64 evaluation within the derived bound, and the
Python classes on CPU tensors: torch's bits, state_dict both ways, schedulers, skipped parameters, get_optimizer."""
import copy
import ctypes
import re

import numpy as np
import pytest
import torch
from torch import nn

import adam_reference as R

WORD = 8


@pytest.fixture(scope="module")
def L():
    from ssl_amd import _lib
    return _lib.lib()


def _arr(values):
    return np.ascontiguousarray(values, dtype=np.uintp)


def _fill(L, p, g, m, v, counts):
    p, g, m, v, c = (_arr(x) for x in (p, g, m, v, counts))
    nbytes = L.ssg_adam_table_bytes(len(c), c.ctypes.data)
    table, grads = np.zeros(nbytes // WORD, dtype=np.uint64), np.zeros(max(len(c), 1), dtype=np.uint64)
    rc = L.ssg_adam_table_fill(len(c), p.ctypes.data, g.ctypes.data, m.ctypes.data, v.ctypes.data, c.ctypes.data,
                               table.ctypes.data, nbytes, grads.ctypes.data, WORD * len(c))
    return rc, table, grads[:len(c)]


# ---- the C ABI ----
def test_symbols_have_the_headers_prototypes(L):
    from ssl_amd import _lib, optim
    size_t, ptr, i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
    want = {"ssg_adam_table_bytes": (size_t, [size_t, ptr]),
            "ssg_adam_table_fill": (i, [size_t, ptr, ptr, ptr, ptr, ptr, ptr, size_t, ptr, size_t]),
            "ssg_adam_grads_fill": (i, [ptr, size_t, ptr, ptr, size_t]),
            "ssg_adam_apply": (i, [ptr, ptr, size_t, ptr, ptr])}
    for name, proto in want.items():
        assert _lib.PROTOTYPES[name] == proto, name
        assert getattr(L, name).argtypes == proto[1]
    assert [_lib.CONSTANTS["SSG_ADAM_" + k] for k in ("PLAIN", "L2", "DECOUPLED")] == [R.PLAIN, R.L2, R.DECOUPLED]
    assert (optim.PLAIN, optim.L2, optim.DECOUPLED) == (R.PLAIN, R.L2, R.DECOUPLED)
    assert L.ssg_abi_version() == 6
    # the binding's record is the header's: the same members in the same order, floats then the int
    with open(_lib.HEADER) as f:
        body = re.search(r"typedef struct ssg_adam_scalars \{(.*?)\} ssg_adam_scalars;", f.read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [(t, n.strip()) for t, names in re.findall(r"\b(float|int) ([^;]+);", body) for n in names.split(",")]
    ctype = {"float": ctypes.c_float, "int": ctypes.c_int}
    assert [(n, ctype[t]) for t, n in members] == list(optim.Scalars._fields_)
    assert ctypes.sizeof(optim.Scalars) == 36


@pytest.mark.parametrize("residue", [0, 4, 8, 12])
def test_table_covers_every_element_once_in_order(L, residue):
    chunk = L.ssg_multi_chunk()
    counts = [0, 1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 7]
    k = len(counts)
    p = [0x1000000 * (i + 1) + residue for i in range(k)]
    g = [0x20000000 + 0x1000000 * i + (residue + 4 * i) % 16 for i in range(k)]
    m = [0x40000000 + 0x1000000 * i + 4 * (i % 4) for i in range(k)]
    v = [0x60000000 + 0x1000000 * i + 12 for i in range(k)]
    rc, table, grads = _fill(L, p, g, m, v, counts)
    assert rc == 0
    n_chunks = sum(-(-n // chunk) for n in counts)
    assert L.ssg_multi_chunks(k, _arr(counts).ctypes.data) == n_chunks
    assert table.size == 4 + 4 * k + n_chunks
    assert table[:4].tolist() == [k, n_chunks, chunk, 0]
    assert table[4:4 + 4 * k].reshape(-1, 4).tolist() == [list(r) for r in zip(p, m, v, counts)]
    assert grads.tolist() == g
    covered = []
    for w in table[4 + 4 * k:].tolist():
        t, c = w >> 32, w & 0xffffffff
        assert t < k and c * chunk < counts[t]
        covered.append((t, c * chunk, min(counts[t], (c + 1) * chunk)))
    assert covered == [(t, o, min(n, o + chunk)) for t, n in enumerate(counts) for o in range(0, n, chunk)]
    # new gradient addresses cost the array alone
    g2 = [a + 0x800000 for a in g]
    again = np.zeros(k, dtype=np.uint64)
    before = table.copy()
    assert L.ssg_adam_grads_fill(table.ctypes.data, k, _arr(g2).ctypes.data, again.ctypes.data, WORD * k) == 0
    assert again.tolist() == g2 and np.array_equal(table, before)


def test_an_empty_set_is_a_header(L):
    rc, table, grads = _fill(L, [], [], [], [], [])
    assert rc == 0 and table.tolist() == [0, 0, L.ssg_multi_chunk(), 0]
    rc, table, grads = _fill(L, [0, 0], [0, 0], [0, 0], [0, 0], [0, 0])        # empty tensors: pointers unused
    assert rc == 0 and table[:2].tolist() == [2, 0] and table.size == 4 + 8


def test_every_refusal_leaves_the_arguments_untouched(L):
    from ssl_amd import _lib, optim
    C = _lib.CONSTANTS
    chunk = L.ssg_multi_chunk()
    good = dict(p=[0x1000, 0x2000], g=[0x3000, 0x4000], m=[0x5000, 0x6000], v=[0x7000, 0x8000], c=[5, 7])
    c = _arr(good["c"])
    nbytes = L.ssg_adam_table_bytes(2, c.ctypes.data)
    assert nbytes == WORD * (4 + 8 + 2)
    table = np.full(nbytes // WORD + 1, 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    grads = np.full(3, 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    t0, g0 = table.copy(), grads.copy()

    def fill(t_=table.ctypes.data, b_=nbytes, gr_=grads.ctypes.data, gb_=2 * WORD, **kw):
        a = {k: (None if kw.get(k, 0) is None else _arr(kw.get(k, good[k]))) for k in good}
        held.append((a, {k: None if x is None else x.copy() for k, x in a.items()}))
        ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
        return L.ssg_adam_table_fill(2, ptr(a["p"]), ptr(a["g"]), ptr(a["m"]), ptr(a["v"]), ptr(a["c"]), t_, b_, gr_, gb_)

    held = []
    assert fill(t_=None) == fill(gr_=None) == C["SSG_E_BADARG"]
    for k in good:
        assert fill(**{k: None}) == C["SSG_E_BADARG"], k
    for k in "pgmv":
        assert fill(**{k: [0, good[k][1]]}) == C["SSG_E_BADARG"], k           # a null address of a non-empty tensor
        for off in (1, 2, 3):
            assert fill(**{k: [good[k][0], good[k][1] + off]}) == C["SSG_E_ALIGN"], (k, off)
    assert fill(t_=table.ctypes.data + 4) == fill(gr_=grads.ctypes.data + 4) == C["SSG_E_ALIGN"]
    assert fill(b_=nbytes - 1) == fill(gb_=2 * WORD - 1) == C["SSG_E_WORKSPACE"]
    # overlap: the same tensor twice, g inside m, one element shared by v of one tensor and p of the next, p == g
    assert fill(p=[0x1000, 0x1000]) == C["SSG_E_BADARG"]
    assert fill(g=[0x5008, 0x4000]) == C["SSG_E_BADARG"]
    assert fill(v=[0x2000 - 16, 0x8000]) == C["SSG_E_BADARG"]
    assert fill(g=[0x1000, 0x4000]) == C["SSG_E_BADARG"]
    assert fill(v=[0x2000 - 20, 0x8000]) == 0                                   # (touching is no overlap)
    table[:], grads[:] = t0, g0
    huge = [5, chunk << 31]                                                      # 2^31 chunks: no int holds the count
    assert fill(c=huge) == C["SSG_E_TOOLARGE"]
    assert L.ssg_adam_table_bytes(2, _arr(huge).ctypes.data) == 0
    assert L.ssg_multi_chunks(2, _arr(huge).ctypes.data) == 2 ** 31
    assert np.array_equal(table, t0) and np.array_equal(grads, g0)
    assert all(a[k] is None or np.array_equal(a[k], was[k]) for a, was in held for k in good)
    assert fill() == 0 and table[-1] == t0[-1] and grads[-1] == g0[-1] and table[1] == 2
    # ssg_adam_grads_fill: the same checks of the new addresses against the image's p, m and v
    filled, gfilled = table.copy(), grads.copy()
    t = table.ctypes.data
    move = lambda g_, t_=t, n_=2, out_=grads.ctypes.data, b_=2 * WORD: L.ssg_adam_grads_fill(  # noqa: E731
        t_, n_, None if g_ is None else g_.ctypes.data, out_, b_)
    ok = _arr([0x9000, 0xa000])
    assert move(ok, t_=None) == move(None) == move(ok, out_=None) == C["SSG_E_BADARG"]
    assert move(ok, n_=3) == C["SSG_E_BADARG"]                                  # the image of another set
    assert move(_arr([0, 0xa000])) == C["SSG_E_BADARG"]
    assert move(_arr([0x9002, 0xa000])) == C["SSG_E_ALIGN"]
    assert move(ok, t_=t + 4) == move(ok, out_=grads.ctypes.data + 4) == C["SSG_E_ALIGN"]
    assert move(_arr([0x5004, 0xa000])) == C["SSG_E_BADARG"]                    # inside m of tensor 0
    assert move(_arr([0x9000, 0x9010])) == C["SSG_E_BADARG"]                    # the new gradients overlap each other
    assert move(ok, b_=2 * WORD - 1) == C["SSG_E_WORKSPACE"]
    assert np.array_equal(table, filled) and np.array_equal(grads, gfilled) and ok.tolist() == [0x9000, 0xa000]
    assert move(ok) == 0 and grads[:2].tolist() == [0x9000, 0xa000] and grads[2] == g0[2]
    # ssg_adam_apply: every refusal is decided before the launch (no device is touched: the images are host memory)
    s = optim.scalars(1e-3, 0.9, 0.99, 1e-8, 0.0, False, 1.0)
    sp, gp = ctypes.addressof(s), grads.ctypes.data
    before = bytes(s)
    assert L.ssg_adam_apply(None, gp, 2, sp, None) == L.ssg_adam_apply(t, None, 2, sp, None) \
        == L.ssg_adam_apply(t, gp, 2, None, None) == C["SSG_E_BADARG"]
    for mode in (-1, 3):
        bad = optim.scalars(1e-3, 0.9, 0.99, 1e-8, 0.0, False, 1.0)
        bad.mode = mode
        assert L.ssg_adam_apply(t, gp, 2, ctypes.addressof(bad), None) == C["SSG_E_BADARG"]
    assert L.ssg_adam_apply(t + 4, gp, 2, sp, None) == L.ssg_adam_apply(t, gp + 4, 2, sp, None) == C["SSG_E_ALIGN"]
    buf = (ctypes.c_char * 48)()
    odd = ctypes.addressof(buf) + 2
    ctypes.memmove(odd, sp, 36)
    assert L.ssg_adam_apply(t, gp, 2, odd, None) == C["SSG_E_ALIGN"]
    assert L.ssg_adam_apply(t, gp, 2 ** 31, sp, None) == C["SSG_E_TOOLARGE"]
    assert L.ssg_adam_apply(t, gp, 0, sp, None) == 0                            # nothing to launch
    assert bytes(s) == before and np.array_equal(table, filled)


# ---- the restatement and torch's CPU Adam against the fp64 evaluation ----
def _torch_step(p, g, m, v, lr, betas, eps, wd, decoupled, step):
    """One step of torch's foreach=False CPU Adam / AdamW from the given state: (p, m, v) as numpy."""
    P = nn.Parameter(torch.from_numpy(p.copy()))
    P.grad = torch.from_numpy(g.copy())
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([P], lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    opt.state[P] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(m.copy()),
                        exp_avg_sq=torch.from_numpy(v.copy()))
    opt.step()
    assert float(opt.state[P]["step"]) == step
    return P.detach().numpy(), opt.state[P]["exp_avg"].numpy(), opt.state[P]["exp_avg_sq"].numpy()


@pytest.mark.parametrize("step", [1, 2, 10 ** 6])
@pytest.mark.parametrize("betas", [(0.9, 0.99), (0.9, 0.999)])
@pytest.mark.parametrize("wd,decoupled", [(0.0, False), (0.01, False), (0.01, True)])
def test_restatement_and_torch_meet_the_bound_against_fp64(wd, decoupled, betas, step):
    rng = np.random.default_rng(1000 * step % 977 + int(1e4 * betas[1]) + (2 if decoupled else bool(wd)))
    n, lr, eps = 40000, 2e-4, 1e-8
    p, m, v = R.state_at(rng, n, step, *betas)
    g = R.gradients(rng, n)
    s = R.host_scalars(lr, betas[0], betas[1], eps, wd, decoupled, float(step))
    assert s["mode"] == (R.PLAIN if wd == 0 else R.DECOUPLED if decoupled else R.L2)
    want, bound = R.exact_and_bound(p, g, m, v, s)
    _, faithful = R.exact_and_bound(p, g, m, v, s, sqrt_ulps=1.0)     # torch's CPU square root is faithfully rounded
    ours = R.restate(p, g, m, v, s)
    theirs = _torch_step(p, g, m, v, lr, betas, eps, wd, decoupled, step)
    sg = np.abs(g.astype(np.float64)) + s["wd"] * np.abs(p.astype(np.float64))
    scale = {"m": np.abs(m.astype(np.float64)) + sg, "v": np.abs(v.astype(np.float64)) + sg ** 2}
    for k, name in enumerate(("p", "m", "v")):
        a, b = R.share(ours[k], want[k], bound[k]), R.share(theirs[k], want[k], faithful[k])
        line = f"{name}: share of the bound used: restatement {a:.3f}, torch's CPU result {b:.3f}"
        if name in scale:
            line += (f"; in units of 2^-24 scale: {R.units(ours[k], want[k], scale[name]):.2f}, "
                     f"{R.units(theirs[k], want[k], scale[name]):.2f}")
        print(line + f"; equal bits {float((R.bits(ours[k]) == R.bits(theirs[k])).mean()):.3f}")
        assert a <= 1.0 and b <= 1.0, (name, a, b)
    assert not R.same_bits(want[0].astype(np.float32), p)                       # the step moved the parameters


def test_the_bound_is_not_proportional_to_the_update():
    """m cancels inside the lerp: with m = -g w1 / (1 - w1)... the new m is 0 and so is the update, while m's rounding
    is of the size of u (|m| + |g|); the bound of p must leave room for a e(m) / den, and does."""
    rng = np.random.default_rng(7)
    g = R.gradients(rng, 5000)
    m = (-g.astype(np.float64) * 0.1 / 0.9).astype(np.float32)
    v = (g.astype(np.float64) ** 2).astype(np.float32)
    p = np.zeros_like(g)
    s = R.host_scalars(2e-4, 0.9, 0.99, 1e-8, 0.0, False, 10.0)
    want, bound = R.exact_and_bound(p, g, m, v, s)
    ours = R.restate(p, g, m, v, s)
    update = np.abs(want[0])
    assert float(np.median(bound[0] / (R.U * np.maximum(update, 1e-300)))) > 100.0
    assert R.share(ours[0], want[0], bound[0]) <= 1.0


# ---- the Python classes on CPU tensors ----
def _net(seed=0, dtype=torch.float32):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Conv2d(3, 5, 3), nn.PReLU(), nn.Conv2d(5, 2, 1, bias=False), nn.Linear(7, 3)).to(dtype)


def _set_grads(nets, gen, skip=()):
    for i, ps in enumerate(zip(*(n.parameters() for n in nets))):
        g = torch.randn(ps[0].shape, generator=gen, dtype=ps[0].dtype)
        for p in ps:
            p.grad = None if i in skip else g.clone()


def _same(a, b):
    return all(R.same_bits(p.detach().numpy(), q.detach().numpy()) for p, q in zip(a.parameters(), b.parameters()))


def _same_state(a, b, na, nb):
    for p, q in zip(na.parameters(), nb.parameters()):
        sa, sb = a.state.get(p, {}), b.state.get(q, {})
        if set(sa) != set(sb) or any(not torch.equal(sa[k], sb[k]) for k in sa):
            return False
    return True


@pytest.mark.parametrize("name,kwargs", [("Adam", dict(betas=(0.9, 0.99))), ("Adam", dict(weight_decay=0.01)),
                                         ("AdamW", dict()), ("AdamW", dict(weight_decay=0.0)),
                                         ("Adam", dict(amsgrad=True)), ("Adam", dict(maximize=True, foreach=False))])
def test_classes_on_cpu_tensors_equal_torchs_bits(name, kwargs):
    from ssl_amd import optim
    a, b = _net(), _net()
    ours, theirs = getattr(optim, name)(a.parameters(), 1e-3, **kwargs), getattr(torch.optim, name)(b.parameters(), 1e-3, **kwargs)
    assert isinstance(ours, getattr(torch.optim, name)) and ours.defaults == theirs.defaults
    gen = torch.Generator().manual_seed(3)
    for _ in range(4):
        _set_grads((a, b), gen)
        assert ours.step(lambda: 1.5) == 1.5
        theirs.step()
    assert _same(a, b) and _same_state(ours, theirs, a, b)
    assert all(float(ours.state[p]["step"]) == 4.0 and not ours.state[p]["step"].is_cuda for p in a.parameters())


def test_state_dict_round_trips_both_ways_and_steps_on():
    from ssl_amd import optim
    gen = torch.Generator().manual_seed(5)
    a, b = _net(), _net()
    ours, theirs = optim.Adam(a.parameters(), 1e-3, betas=(0.9, 0.99)), torch.optim.Adam(b.parameters(), 1e-3, betas=(0.9, 0.99))
    for _ in range(2):
        _set_grads((a, b), gen)
        ours.step()
        theirs.step()
    sd_ours, sd_theirs = copy.deepcopy(ours.state_dict()), copy.deepcopy(theirs.state_dict())
    assert sd_ours["param_groups"] == sd_theirs["param_groups"] and sd_ours["state"].keys() == sd_theirs["state"].keys()
    # each checkpoint into the OTHER class, on fresh copies of the weights
    c, d = copy.deepcopy(a), copy.deepcopy(b)
    into_ours, into_theirs = optim.Adam(c.parameters(), 1e-3), torch.optim.Adam(d.parameters(), 1e-3)
    into_ours.load_state_dict(sd_theirs)
    into_theirs.load_state_dict(sd_ours)
    twin = copy.deepcopy(ours)                               # a copy carries no table
    assert "_plans" not in twin.__dict__ or twin._plans == {}
    for _ in range(2):
        _set_grads((a, b, c, d), gen)
        for o in (ours, theirs, into_ours, into_theirs):
            o.step()
    assert _same(a, b) and _same(c, b) and _same(d, b)
    assert _same_state(into_ours, theirs, c, b) and _same_state(into_theirs, theirs, d, b)
    assert float(into_ours.state[next(c.parameters())]["step"]) == 4.0
    # AdamW's checkpoint loads into Adam and back: the group's decoupled_weight_decay travels with it
    w = optim.AdamW(_net().parameters(), 1e-3)
    plain = optim.Adam(_net().parameters(), 1e-3)
    plain.load_state_dict(w.state_dict())
    assert plain.param_groups[0]["decoupled_weight_decay"] is True


class _Counting:
    """The library with ssg_adam_apply counted and done on the host: CPU tensors are declared native and the images stay
    on the host, so the counted apply reads them and runs the restatement on the tensors' memory."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        return getattr(self.real, name)

    def ssg_adam_apply(self, table, grads, n_chunks, scalars, stream):
        from ssl_amd import optim
        s = optim.Scalars.from_address(scalars)
        words = np.ctypeslib.as_array(ctypes.cast(table, ctypes.POINTER(ctypes.c_uint64)), (4,))
        nt, nc = int(words[0]), int(words[1])
        assert nc == n_chunks
        records = np.ctypeslib.as_array(ctypes.cast(table, ctypes.POINTER(ctypes.c_uint64)), (4 + 4 * nt,))[4:].reshape(-1, 4)
        gaddr = np.ctypeslib.as_array(ctypes.cast(grads, ctypes.POINTER(ctypes.c_uint64)), (nt,))
        sd = {k: getattr(s, k) for k, _ in optim.Scalars._fields_}
        self.calls.append(dict(sd, tensors=nt))
        view = lambda a, n: np.ctypeslib.as_array(ctypes.cast(int(a), ctypes.POINTER(ctypes.c_float)), (n,))  # noqa: E731
        for (p, m, v, n), g in zip(records.tolist(), gaddr.tolist()):
            if n:
                P, G, M, V = view(p, n), view(g, n), view(m, n), view(v, n)
                P[:], M[:], V[:] = R.restate(P.copy(), G.copy(), M.copy(), V.copy(), sd)
        return 0


@pytest.fixture
def counting(monkeypatch):
    from ssl_amd import optim
    lib = _Counting(optim._lib.lib())
    monkeypatch.setattr(optim, "_library", lambda: lib)
    monkeypatch.setattr(optim, "_on_gpu", lambda t: True)
    monkeypatch.setattr(optim, "_upload", lambda host, device: host.clone())
    return lib


def _module(n_tensors, seed):
    gen = torch.Generator().manual_seed(seed)
    m = nn.Module()
    for i in range(n_tensors):
        shape = (1 + i % 64,) if i % 3 else (2, 1 + i % 7, 3)
        m.register_parameter(f"p{i}", nn.Parameter(torch.randn(shape, generator=gen)))
    return m


@pytest.mark.parametrize("n_tensors", [3, 300])
def test_step_is_one_apply_per_group_whatever_the_number_of_tensors(counting, n_tensors):
    from ssl_amd import optim
    net = _module(n_tensors, n_tensors)
    params = list(net.parameters())
    opt = optim.Adam([dict(params=params[:2]), dict(params=params[2:], lr=5e-4, weight_decay=0.01)], 1e-3, betas=(0.9, 0.99))
    states = {k: (p.detach().numpy().copy(), np.zeros(p.numel(), np.float32).reshape(p.shape),
                  np.zeros(p.numel(), np.float32).reshape(p.shape)) for k, p in net.named_parameters()}
    gen = torch.Generator().manual_seed(9)
    for t in (1, 2, 3):
        _set_grads((net,), gen)
        opt.step()
        assert len(counting.calls) == 2 * t
        first, second = counting.calls[-2:]
        assert (first["tensors"], second["tensors"]) == (2, n_tensors - 2)
        assert (first["mode"], second["mode"]) == (R.PLAIN, R.L2)
        for k, p in net.named_parameters():
            group = 0 if k in ("p0", "p1") else 1
            s = R.host_scalars([1e-3, 5e-4][group], 0.9, 0.99, 1e-8, [0.0, 0.01][group], False, float(t))
            q, m, v = states[k]
            states[k] = R.restate(q, p.grad.numpy(), m, v, s)
    for k, p in net.named_parameters():
        assert R.same_bits(p.detach().numpy(), states[k][0]), k
        assert R.same_bits(opt.state[p]["exp_avg"].numpy(), states[k][1]) and float(opt.state[p]["step"]) == 3.0
        assert R.same_bits(opt.state[p]["exp_avg_sq"].numpy(), states[k][2]), k
    plans = opt._plans
    assert sorted(plans) == [(0, 0), (1, 0)] and all(pl.native and pl.rebuilds == 1 for pl in plans.values())
    assert all(pl.grad_uploads == 2 for pl in plans.values())        # (fresh gradient tensors every step: the array alone)


def test_multisteplr_changes_the_launch_scalar_and_nothing_else(counting):
    from ssl_amd import optim
    net = _module(5, 1)
    opt = optim.Adam(net.parameters(), 2e-4, betas=(0.9, 0.99))
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2], gamma=0.5)
    gen = torch.Generator().manual_seed(2)
    _set_grads((net,), gen)
    grads = [p.grad for p in net.parameters()]
    for t in range(1, 5):
        for g in grads:
            g.copy_(torch.randn(g.shape, generator=gen))
        opt.step()
        sched.step()
    lrs = [2e-4, 2e-4, 1e-4, 1e-4]
    for t, (call, lr) in enumerate(zip(counting.calls, lrs), 1):
        want = R.host_scalars(lr, 0.9, 0.99, 1e-8, 0.0, False, float(t))
        assert call["a"] == float(np.float32(want["a"])) and call["s2"] == float(np.float32(want["s2"]))
        assert all(call[k] == counting.calls[0][k] for k in ("w1", "b2", "w2", "eps", "wd", "cwd", "mode", "tensors"))
    plan = opt._plans[(0, 0)]
    assert plan.rebuilds == 1 and plan.grad_uploads == 0 and len(counting.calls) == 4


def test_a_parameter_without_a_gradient_is_skipped_and_a_later_one_splits_by_step(counting):
    from ssl_amd import optim
    net = _module(6, 4)
    params = list(net.parameters())
    opt = optim.Adam(net.parameters(), 1e-3)
    gen = torch.Generator().manual_seed(6)
    _set_grads((net,), gen, skip=(1, 4))
    opt.step()
    opt.step()
    assert [c["tensors"] for c in counting.calls] == [4, 4]
    assert opt.state.get(params[1], {}) == {} and opt.state.get(params[4], {}) == {}
    assert all(float(opt.state[p]["step"]) == 2.0 for i, p in enumerate(params) if i not in (1, 4))
    before = params[1].detach().clone()
    _set_grads((net,), gen)                                         # now every parameter has one: steps 2 and 0
    opt.step()
    assert sorted(c["tensors"] for c in counting.calls[2:]) == [2, 4] and len(counting.calls) == 4
    by_tensors = {c["tensors"]: c for c in counting.calls[2:]}
    assert by_tensors[4]["a"] == float(np.float32(R.host_scalars(1e-3, 0.9, 0.999, 1e-8, 0, False, 3.0)["a"]))
    assert by_tensors[2]["a"] == float(np.float32(R.host_scalars(1e-3, 0.9, 0.999, 1e-8, 0, False, 1.0)["a"]))
    assert [float(opt.state[p]["step"]) for p in params] == [3.0, 1.0, 3.0, 3.0, 1.0, 3.0]
    assert not torch.equal(params[1].detach(), before)
    # against torch from the same state
    ref_net = copy.deepcopy(net)
    ref = torch.optim.Adam(ref_net.parameters(), 1e-3)
    ref.load_state_dict(copy.deepcopy(opt.state_dict()))
    _set_grads((net, ref_net), gen)
    opt.step()
    ref.step()
    for p, q in zip(net.parameters(), ref_net.parameters()):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-7)
        assert float(opt.state[p]["step"]) == float(ref.state[q]["step"])


def test_overlapping_tensors_and_a_fused_group_are_torchs(counting):
    """Two parameters that share memory: the fill refuses the set, no table exists, and the group runs torch's adam();
    a group that asks for torch's fused implementation is never declared native."""
    from ssl_amd import optim

    def pair():
        base = torch.arange(10, dtype=torch.float32) / 10
        return [nn.Parameter(base[0:6]), nn.Parameter(base[4:10])]

    a, b = pair(), pair()
    ours, theirs = optim.Adam(a, 1e-2), torch.optim.Adam(b, 1e-2)
    gen = torch.Generator().manual_seed(8)
    for _ in range(2):
        for p, q in zip(a, b):
            p.grad = torch.randn(6, generator=gen)
            q.grad = p.grad.clone()
        ours.step()
        theirs.step()
    assert counting.calls == [] and not ours._plans[(0, 0)].native and ours._plans[(0, 0)].table is None
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    net = _module(3, 2)
    _set_grads((net,), gen)
    group = dict(optim.Adam(net.parameters(), 1e-3).param_groups[0], fused=True)
    assert not optim._eligible(group, [], False) and optim._eligible(dict(group, fused=None), [], False)
    assert not optim._eligible(dict(group, fused=None, lr=torch.tensor(1e-3)), [], False)


def test_get_optimizer_names():
    from ssl_amd import optim
    want = {"Adam": optim.Adam, "AdamW": optim.AdamW, "Adamax": torch.optim.Adamax, "SGD": torch.optim.SGD,
            "ASGD": torch.optim.ASGD, "RMSprop": torch.optim.RMSprop, "Rprop": torch.optim.Rprop}
    for name, cls in want.items():
        opt = optim.get_optimizer(name, _net().parameters(), 2e-4)
        assert type(opt) is cls and isinstance(opt, getattr(torch.optim, name)) and opt.param_groups[0]["lr"] == 2e-4
    opt = optim.get_optimizer("Adam", _net().parameters(), 2e-4, weight_decay=0, betas=[0.9, 0.99])    # the yml's form
    assert list(opt.param_groups[0]["betas"]) == [0.9, 0.99] and opt.param_groups[0]["weight_decay"] == 0
    with pytest.raises(NotImplementedError, match="Lion"):
        optim.get_optimizer("Lion", _net().parameters(), 2e-4)
    import ssl_amd
    assert ssl_amd.optim is optim and "optim" in ssl_amd.__all__
