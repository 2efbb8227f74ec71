"""CPU: the one route decision of the W1D host path (losses._route) on meta stand-ins -- a meta tensor is not `is_cuda`, so the decision's
one device test, losses._is_hip_tensor, is patched to take them (as tests/test_f64_host.py does for the float64 gate).  The expected
routes are written by hand from DESIGN.md section 1.1; a second test counts how often one call asks each gate."""
import warnings

import pytest
import torch

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
RS, TIE_FREE = 8, 256    # SOT_FLAG_REQUIRE_SORT, SOT_FLAG_TIE_FREE_GRADIENT
GATES = ("_f64_route_applies", "_hip_domain", "_beyond_one_cu", "mixed_route_applies", "_typed_forward_applies", "_typed_training_applies")


def M(*shape, dtype=F32, grad=False):
    return torch.empty(*shape, dtype=dtype, device="meta", requires_grad=grad)


@pytest.fixture()
def losses(monkeypatch):
    from sot_amd import _native, losses
    _native.load()
    monkeypatch.setattr(losses, "_is_hip_tensor", lambda t: t.device.type == "meta")
    monkeypatch.setattr(losses, "_warned", set())
    return losses


def _pair(n, dtype=F32, B=3, m=None, grad="", pos_dtype=None, rowpos=False):
    """(x, y, xpos, ypos) stand-ins: B rows of n (and m) points on shared grids or per-row positions; grad: which of 'x', 'y', 'p'
    (both position tensors) ask for a gradient."""
    m = n if m is None else m
    pd = F32 if pos_dtype is None else pos_dtype
    pos = (lambda k: M(B, k, dtype=pd, grad="p" in grad)) if rowpos else (lambda k: M(k, dtype=pd, grad="p" in grad))
    return M(B, n, dtype=dtype, grad="x" in grad), M(B, m, dtype=dtype, grad="y" in grad), pos(n), pos(m)


# name -> (arguments of _route after the four tensors, the four tensors, expected (family, dtype, widen, typed_training), warn_once keys)
def _table():
    mixed32 = (M(3, 64), M(3, 8, grad=True), M(64), M(3, 8))
    mixed16 = (M(3, 8, dtype=BF16), M(3, 64, dtype=BF16), M(3, 8), M(64))
    return {
        "f32 shared": ((1, RS), _pair(64, grad="y"), ("rows", F32, False, False), []),
        "f32 per-row positions": ((1, RS), _pair(33, rowpos=True, grad="xyp"), ("rows", F32, False, False), []),
        "f32 return_quantiles": ((1, RS, True), _pair(64, grad="y"), ("rows", F32, False, False), []),
        "f32 mixed supports": ((1, RS), mixed32, ("mixed", F32, False, False), []),
        "f32 mixed supports, return_quantiles": ((1, RS, True), mixed32, ("rows", F32, False, False), []),
        "bf16 no gradient": ((1, RS), _pair(64, BF16), ("rows", BF16, False, False), []),
        "bf16 y gradient, 512 shared": ((1, RS), _pair(512, BF16, grad="y"), ("rows", BF16, False, True), []),
        "bf16 x and y gradient, 512 shared": ((2, RS | 1), _pair(512, BF16, grad="xy"), ("rows", BF16, False, True), []),
        "bf16 y gradient, 257": ((1, RS), _pair(257, BF16, grad="y"), ("rows", F32, True, False), []),
        "bf16 y gradient, tie-free form": ((1, RS | TIE_FREE), _pair(512, BF16, grad="y"), ("rows", F32, True, False), []),
        "bf16 position gradient": ((1, RS), _pair(512, BF16, grad="yp"), ("rows", F32, True, False), []),
        "bf16 per-row positions, gradient": ((1, RS), _pair(512, BF16, grad="y", rowpos=True), ("rows", F32, True, False), []),
        "bf16 return_quantiles": ((1, RS, True), _pair(512, BF16), ("rows", F32, True, False), []),
        "bf16 mixed supports": ((1, RS), mixed16, ("mixed", F32, True, False), []),
        "f64 shared": ((1, RS), _pair(33, F64, pos_dtype=F64, grad="y"), ("f64", F64, False, False), []),
        "f64 per-row": ((1, RS), _pair(33, F64, pos_dtype=F64, rowpos=True), ("f64", F64, False, False), []),
        "f64 on f32 positions": ((1, RS), _pair(33, F64), ("torch", F64, False, False), ["not-hip-f32"]),
        "f64 return_quantiles": ((1, RS, True), _pair(33, F64, pos_dtype=F64), ("torch", F64, False, False), ["not-hip-f32"]),
        "f64 position gradient": ((1, RS), _pair(33, F64, pos_dtype=F64, grad="p"), ("torch", F64, False, False), ["not-hip-f32"]),
        "f32 beyond one CU": ((1, RS), _pair(9001, B=2), ("torch", F32, False, False), ["row-too-long"]),
        "f32 beyond one CU, backward": ((1, RS), _pair(6001, B=2, grad="y"), ("torch", F32, False, False), ["row-too-long"]),
        "f32 6001 without a gradient": ((1, RS), _pair(6001, B=2), ("rows", F32, False, False), []),
        "bf16 beyond one CU": ((1, RS), _pair(9001, BF16, B=2), ("torch", F32, True, False), ["row-too-long"]),
        "CPU tensors": ((1, RS), tuple(torch.empty(s) for s in ((3, 64), (3, 64), (64,), (64,))), ("torch", F32, False, False), []),
        "CPU bf16 tensors": ((1, RS), (torch.empty(3, 64, dtype=BF16), torch.empty(3, 64, dtype=BF16), torch.empty(64), torch.empty(64)),
                             ("torch", BF16, False, False), []),
        "CPU weights on GPU positions": ((1, RS), (torch.empty(3, 64), torch.empty(3, 64), M(64), M(64)), ("torch", F32, False, False), ["not-hip-f32"]),
    }


@pytest.mark.parametrize("name", list(_table()))
def test_route_table(losses, name):
    args, tensors, want, keys = _table()[name]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = losses._route(*tensors, *args)
    assert tuple(got) == want, (name, got)
    assert sorted(losses._warned) == sorted(keys) and len(caught) == len(keys), (name, losses._warned, [str(w.message) for w in caught])


def test_route_follows_the_grad_mode_and_a_trace(losses, monkeypatch):
    x, y, xp, yp = _pair(512, BF16, grad="y")
    assert tuple(losses._route(x, y, xp, yp, 1, RS)) == ("rows", BF16, False, True)
    with torch.no_grad():                                                    # nobody asks for a gradient: the typed forward
        assert tuple(losses._route(x, y, xp, yp, 1, RS)) == ("rows", BF16, False, False)
        assert tuple(losses._route(*_pair(6001, B=2, grad="y"), 1, RS)) == ("rows", F32, False, False)   # ... and the forward's size limit holds
    f64 = _pair(33, F64, pos_dtype=F64, grad="y")
    assert losses._route(*f64, 1, RS).family == "f64"
    monkeypatch.setattr(losses, "_compiling", lambda: True)                  # a call that is being traced
    assert tuple(losses._route(x, y, xp, yp, 1, RS)) == ("rows", F32, True, False)       # no typed training op: widened, the float32 ops
    with torch.no_grad():
        assert tuple(losses._route(x, y, xp, yp, 1, RS)) == ("rows", BF16, False, False)  # the typed forward has ops
    assert tuple(losses._route(*_pair(64, grad="y"), 1, RS)) == ("rows", F32, False, False)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        assert tuple(losses._route(*f64, 1, RS)) == ("torch", F64, False, False)         # the float64 kernels have none
    assert losses._warned == {"not-hip-f32"} and len(caught) == 1


def test_switches_send_calls_back_to_the_older_routes(losses, monkeypatch):
    mixed = (M(3, 64), M(3, 8), M(64), M(3, 8))
    monkeypatch.setattr(losses, "MIXED_ROUTE", False)
    assert losses._route(*mixed, 1, RS).family == "rows"
    monkeypatch.setattr(losses, "F64_ROUTE", False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert losses._route(*_pair(33, F64, pos_dtype=F64), 1, RS).family == "torch"


@pytest.mark.parametrize("dx,dy,dpos,named", [(F16, F16, F32, "float16"), (BF16, F32, F32, "bfloat16"), (F32, BF16, F32, "bfloat16"),
                                              (BF16, F16, F32, "bfloat16"), (BF16, BF16, BF16, "bfloat16")],
                         ids=["half", "bf16-f32", "f32-bf16", "bf16-half", "bf16-positions"])
def test_refusals_keep_their_text(losses, dx, dy, dpos, named):
    with pytest.raises(TypeError) as err:
        losses._route(M(3, 64, dtype=dx), M(3, 64, dtype=dy), M(64, dtype=dpos), M(64), 1, RS)
    assert str(err.value) == f"sot_amd computes in float32; got torch.{named} (convert with .float())"
    assert not losses._warned                                                # refused before anything is said


def test_the_float64_gate_is_asked_before_the_domain_gate_can_warn(losses, monkeypatch):
    order = []
    real64, real_dom = losses._f64_route_applies, losses._hip_domain
    monkeypatch.setattr(losses, "_f64_route_applies", lambda *a, **k: (order.append("f64"), real64(*a, **k))[1])
    monkeypatch.setattr(losses, "_hip_domain", lambda *a, **k: (order.append("domain"), real_dom(*a, **k))[1])
    assert losses._route(*_pair(33, F64, pos_dtype=F64), 1, RS).family == "f64"
    assert order == ["f64"] and not losses._warned
    assert losses._route(*_pair(64), 1, RS).family == "rows"                 # float32 weights never ask the float64 gate
    assert order == ["f64", "domain"]


def test_no_gate_runs_twice_in_one_call(losses, monkeypatch):
    """One forward (default, and with dims), one row_losses and one wasserstein_1d on bfloat16 stand-ins that ask for a gradient -- the
    calls that ask every gate.  What comes after the decision is stubbed: stand-ins have no memory to launch on.  _is_shared_row and
    _is_hip_tensor are per-tensor helpers of the gates, not gates of a call, and are not counted."""
    counts = {}
    for name in GATES:
        real = getattr(losses, name)
        monkeypatch.setattr(losses, name, (lambda real, name: lambda *a, **k: (counts.__setitem__(name, counts.get(name, 0) + 1), real(*a, **k))[1])(real, name))
    flag_words = []
    real_flag_word = losses.Wasserstein1D._flag_word
    monkeypatch.setattr(losses.Wasserstein1D, "_flag_word", lambda self, kw: (flag_words.append(1), real_flag_word(self, kw))[1])
    routes = []
    monkeypatch.setattr(losses, "_native_row_losses", lambda route, *a, **k: (routes.append(route), M(3))[1])
    monkeypatch.setattr(losses.Wasserstein1D, "_fused_mean", lambda self, route, *a, **k: (routes.append(route), M(()))[1])
    mod = losses.Wasserstein1D(p=1)
    x, y, xp, yp = _pair(512, BF16, grad="y")
    calls = {
        "forward": lambda: mod(x, y, x_pos=xp, y_pos=yp),
        "forward dims": lambda: mod(x, y, x_pos=xp, y_pos=yp, dims=0),
        "row_losses": lambda: mod.row_losses(x, y, x_pos=xp, y_pos=yp),
        "wasserstein_1d": lambda: losses.wasserstein_1d(xp.expand(3, -1), yp.expand(3, -1), x, y),
    }
    for name, call in calls.items():
        counts.clear()
        flag_words.clear()
        call()
        assert counts == {g: 1 for g in GATES if g != "_f64_route_applies"}, (name, counts)   # bfloat16: every gate but the float64 one, once
        assert len(flag_words) == (0 if name == "wasserstein_1d" else 1), name
    assert [tuple(r) for r in routes] == [("rows", BF16, False, True)] * 3 + [("rows", F32, True, False)]   # (expanded grids are 2-D: widened)
    counts.clear()
    mod(*_pair(33, F64, pos_dtype=F64)[:2], x_pos=M(33, dtype=F64), y_pos=M(33, dtype=F64), dims=0)
    assert counts == {"_f64_route_applies": 1}
