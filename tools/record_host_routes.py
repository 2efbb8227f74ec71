"""Record what the host path of the W1D loss does for a fixed lattice of calls on real GPU tensors: per case the ordered names of the
work-enqueuing callables reached (those of sot_amd._native, _torch_path.module_forward / transport_rows and the C++ host path's
mean_loss / mean_loss_fresh), the grad_fn class of the result, its dtype and shape, the warn_once keys raised and -- unless the call
took the torch-op composition -- the SHA-256 of the loss bytes and of every returned gradient (the kernels sum in a fixed order and use
no atomics, so these are bit-stable).  tests/golden/host_routes.json is this tool's output at the commit before the host-route
refactor; tests/test_host_routes_gpu.py replays the lattice and compares.

    python tools/record_host_routes.py out.json
"""
import hashlib
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NATIVE_NAMES = (
    "PositionPlan", "forward_rows", "loss_fused", "loss_and_grad", "backward_rows", "rows_to_f32", "rows_to_bf16", "forward_rows_bf16",
    "loss_fused_bf16", "backward_rows_bf16", "loss_and_grad_bf16", "forward_rows_f64", "backward_rows_f64", "scale_inplace", "reduce_mean",
    "position_grads", "mixed_forward_rows", "mixed_backward_rows", "mixed_position_grad", "quantiles", "quantiles_backward")
COMPOSITION = ("module_forward", "transport_rows")
GLUE_NAMES = ("mean_loss", "mean_loss_fresh")
ENTRIES = ("forward", "forward_dims0", "forward_hinge", "row_losses", "wasserstein_1d", "forward_rq")
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
HINGE = 0.015   # inside the range of the lattice's row losses (0.010 ... 0.17): some rows are clipped, some are not


def _rows(gen, shape, dtype):
    return (torch.rand(shape, generator=gen, dtype=torch.float64) + 0.01).to(dtype)


def _grid(n, dtype=F32):
    return torch.linspace(0, 1, n, dtype=torch.float64).to(dtype)


def _kind_inputs(kind, gen):
    """(x, y, xpos, ypos) on the CPU for one row of the lattice; a position tensor of kind 'expanded' is expanded after the move."""
    if kind in ("f32_shared", "bf16_64"):
        dt = F32 if kind == "f32_shared" else BF16
        return _rows(gen, (3, 64), dt), _rows(gen, (3, 64), dt), _grid(64), _grid(64)
    if kind == "f32_unsorted":
        order = torch.randperm(64, generator=gen)
        return _rows(gen, (3, 64), F32), _rows(gen, (3, 64), F32), _grid(64)[order], _grid(64)[order]
    if kind == "f32_rowpos":
        return _rows(gen, (3, 33), F32), _rows(gen, (3, 33), F32), _rows(gen, (3, 33), F32), _rows(gen, (3, 33), F32)
    if kind == "f32_expanded":
        return _rows(gen, (3, 33), F32), _rows(gen, (3, 33), F32), _grid(33), _grid(33)
    if kind == "f32_3d":
        return _rows(gen, (2, 2, 33), F32), _rows(gen, (2, 2, 33), F32), _grid(33), _grid(33)
    if kind in ("bf16_512", "bf16_512_pos", "bf16_512_off"):
        return _rows(gen, (3, 512), BF16), _rows(gen, (3, 512), BF16), _grid(512), _grid(512)
    if kind == "bf16_257":
        return _rows(gen, (3, 257), BF16), _rows(gen, (3, 257), BF16), _grid(257), _grid(257)
    if kind.startswith("mixed_"):
        dt = BF16 if kind.endswith("bf16") else F32
        wide, narrow = (_rows(gen, (3, 64), dt), _grid(64)), (_rows(gen, (3, 8), dt), _rows(gen, (3, 8), F32))
        (x, xp), (y, yp) = (wide, narrow) if "_x_" in kind else (narrow, wide)
        return x, y, xp, yp
    if kind in ("f64_shared", "f64_unsorted", "f64_f32pos"):
        order = torch.randperm(33, generator=gen) if kind == "f64_unsorted" else torch.arange(33)
        pdt = F32 if kind == "f64_f32pos" else F64
        return _rows(gen, (3, 33), F64), _rows(gen, (3, 33), F64), _grid(33, pdt)[order], _grid(33, pdt)[order]
    if kind == "f64_rowpos":
        return _rows(gen, (3, 33), F64), _rows(gen, (3, 33), F64), _rows(gen, (3, 33), F64), _rows(gen, (3, 33), F64)
    if kind in ("long_9001", "long_6001"):
        n = int(kind[-4:])
        return _rows(gen, (2, n), F32), _rows(gen, (2, n), F32), _grid(n), _grid(n)
    raise KeyError(kind)


# kind -> the gradient modes its route admits ("none": under torch.no_grad; "y" / "xy": weights; "pos": y and both position tensors)
LATTICE = {
    "f32_shared": ("none", "y", "xy", "pos"), "f32_unsorted": ("none", "y", "xy", "pos"), "f32_rowpos": ("none", "y", "xy", "pos"),
    "f32_expanded": ("none", "y", "xy", "pos"), "f32_3d": ("none", "y", "xy", "pos"),
    "bf16_64": ("none", "y", "xy"), "bf16_512": ("y", "xy"), "bf16_257": ("y", "xy"), "bf16_512_pos": ("pos",), "bf16_512_off": ("none", "y"),
    "mixed_x_f32": ("none", "y", "xy", "pos"), "mixed_y_f32": ("none", "y", "xy", "pos"),
    "mixed_x_bf16": ("none", "y", "xy", "pos"), "mixed_y_bf16": ("none", "y", "xy", "pos"),
    "f64_shared": ("none", "y", "xy"), "f64_rowpos": ("none", "y"), "f64_unsorted": ("none", "y"), "f64_f32pos": ("none", "y"),
    "long_9001": ("none",), "long_6001": ("y",),
}


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


class Recorder:
    """Wraps the callables for the time of one case; names: the ordered list of those reached; keys: the warn_once keys raised."""

    def __init__(self):
        from sot_amd import _native as nat, _torch_path as tp, losses
        self.nat, self.tp, self.losses = nat, tp, losses
        self.names, self.keys, self._saved = [], [], []

    def _wrap(self, owner, name, label=None):
        real = getattr(owner, name)
        label = label or name

        def recorded(*a, **k):
            self.names.append(label)
            return real(*a, **k)
        self._saved.append((owner, name, real))
        setattr(owner, name, recorded)

    def __enter__(self):
        losses = self.losses
        self._state = [(c, list(c)) for c in (losses._functional_plans.entries, losses._f64_grids.entries)]
        self._warned = set(losses._warned)   # every case starts from empty caches and no warning given; __exit__ puts all of it back
        losses._warned.clear()
        for c, _ in self._state:
            c.clear()
        for name in NATIVE_NAMES:
            self._wrap(self.nat, name)
        for name in COMPOSITION:
            self._wrap(self.tp, name)
        glue = self.nat.glue()
        assert glue is not None, "the C++ host path is part of the record: build it first"
        for name in GLUE_NAMES:
            if hasattr(glue, name):
                self._wrap(glue, name)
        real_warn = losses.warn_once

        def warn_once(key, message):
            if key not in losses._warned:
                self.keys.append(repr(key))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                real_warn(key, message)
        self._saved.append((losses, "warn_once", real_warn))
        losses.warn_once = warn_once
        return self

    def __exit__(self, *exc):
        for owner, name, real in reversed(self._saved):
            setattr(owner, name, real)
        self._saved.clear()
        self.losses._warned.clear()
        self.losses._warned.update(self._warned)
        for c, items in self._state:
            c[:] = items


def _call(entry, mod, x, y, xp, yp):
    from sot_amd.losses import wasserstein_1d
    if entry == "wasserstein_1d":
        u = xp if xp.ndim == 2 else xp.expand(x.shape[0], -1)
        v = yp if yp.ndim == 2 else yp.expand(y.shape[0], -1)
        return wasserstein_1d(u, v, x, y, p=1)
    if entry == "row_losses":
        return mod.row_losses(x, y, x_pos=xp, y_pos=yp)
    kw = {"forward": {}, "forward_dims0": {"dims": 0}, "forward_hinge": {"hinge": HINGE}, "forward_rq": {"return_quantiles": True}}[entry]
    return mod(x, y, x_pos=xp, y_pos=yp, **kw)


def _describe(out, rec, leaves):
    outs = list(out) if isinstance(out, (list, tuple)) else [out]
    composition = any(n in COMPOSITION for n in rec.names)
    entry = {"names": list(rec.names), "grad_fn": type(outs[0].grad_fn).__name__ if outs[0].grad_fn is not None else None,
             "dtype": [str(o.dtype) for o in outs], "shape": [list(o.shape) for o in outs], "warn_keys": list(rec.keys)}
    if not composition:
        entry["loss_sha256"] = [_sha(o) for o in outs]
        entry["grad_sha256"] = {name: _sha(t.grad) for name, t in leaves.items() if t.grad is not None}
    else:
        entry["grads"] = sorted(name for name, t in leaves.items() if t.grad is not None)
    return entry


def _backward(out):
    """A fixed non-trivial cotangent for every output that is attached to autograd."""
    outs = [o for o in (out if isinstance(out, (list, tuple)) else [out]) if o.requires_grad]
    if not outs:
        return
    total = None
    for o in outs:
        w = torch.linspace(0.5, 1.5, max(o.numel(), 2), device=o.device, dtype=torch.float64)[:o.numel()].reshape(o.shape).to(o.dtype)
        total = (o * w).sum() if total is None else total + (o * w).sum().to(total.dtype)
    total.backward()


def _one_case(dev, kind, mode, entry, seed):
    from sot_amd import losses
    gen = torch.Generator().manual_seed(seed)
    x, y, xp, yp = (t.to(dev) for t in _kind_inputs(kind, gen))
    leaves = {"x": x, "y": y, "xpos": xp, "ypos": yp}
    if kind == "bf16_512_off":   # rows that start 2 bytes off the 16-byte alignment of a fresh allocation
        flat = {k: torch.zeros(3 * 512 + 1, dtype=BF16, device=dev) for k in ("x", "y")}
        for k, src in (("x", x), ("y", y)):
            flat[k][1:] = src.reshape(-1)
        leaves.update(flat)
    y_leaf, x_leaf = leaves["y"], leaves["x"]
    if mode in ("y", "xy", "pos"):
        y_leaf.requires_grad_(True)
    if mode == "xy":
        x_leaf.requires_grad_(True)
    if mode == "pos":
        xp.requires_grad_(True)
        yp.requires_grad_(True)
    if kind == "bf16_512_off":
        x, y = leaves["x"][1:].view(3, 512), leaves["y"][1:].view(3, 512)
    if kind == "f32_expanded":
        xp, yp = xp.expand(3, -1), yp.expand(3, -1)
    mod = losses.Wasserstein1D(p=1, hinge=(entry == "forward_hinge")).to(dev)
    with Recorder() as rec:   # (a call that raises ends the recording: the lattice holds supported calls only)
        if mode == "none":
            with torch.no_grad():
                out = _call(entry, mod, x, y, xp, yp)
        else:
            out = _call(entry, mod, x, y, xp, yp)
            rec.names.append("--backward--")
            _backward(out)
        if dev.type == "cuda":
            torch.cuda.synchronize()
        return _describe(out, rec, leaves)


def _hot_cases(dev):
    """The module's default call twice: with the same grid tensors (the second call is the recognised hot call), with fresh grid tensors
    (the fresh-positions branch), and both with EARLY_GRADIENT off; each without a gradient and with one for y."""
    from sot_amd import losses
    out = {}
    for early in (True, False):
        for grids in ("same", "fresh"):
            for mode in ("none", "y", "xy"):
                gen = torch.Generator().manual_seed(7)
                x, y = _rows(gen, (3, 64), F32).to(dev), _rows(gen, (3, 64), F32).to(dev)
                leaves = {"x": x, "y": y}
                if mode != "none":
                    y.requires_grad_(True)
                if mode == "xy":
                    x.requires_grad_(True)
                pos = _grid(64).to(dev), _grid(64).to(dev)
                mod = losses.Wasserstein1D(p=1).to(dev)
                saved = losses.EARLY_GRADIENT
                losses.EARLY_GRADIENT = early
                try:
                    with Recorder() as rec:
                        for call in range(2):
                            xp, yp = pos if grids == "same" else (_grid(64).to(dev), _grid(64).to(dev))
                            rec.names.append(f"--call {call}--")
                            if mode == "none":
                                with torch.no_grad():
                                    loss = mod(x, y, x_pos=xp, y_pos=yp)
                            else:
                                loss = mod(x, y, x_pos=xp, y_pos=yp)
                                rec.names.append("--backward--")
                                loss.backward()
                        if dev.type == "cuda":
                            torch.cuda.synchronize()
                        out[f"hot/{'early' if early else 'late'}/{grids}/{mode}"] = _describe(loss, rec, leaves)
                finally:
                    losses.EARLY_GRADIENT = saved
    # bfloat16 training with EARLY_GRADIENT off: the typed forward + mean and the typed backward with the late arguments
    saved = losses.EARLY_GRADIENT
    losses.EARLY_GRADIENT = False
    try:
        out["late/bf16_512/y/forward"] = _one_case(dev, "bf16_512", "y", "forward", 11)
    finally:
        losses.EARLY_GRADIENT = saved
    return out


def record(dev=None):
    """{case name: record} for the whole lattice."""
    dev = dev or torch.device("cuda:0")
    out = {}
    for k, (kind, modes) in enumerate(LATTICE.items()):
        for mode in modes:
            for entry in ENTRIES:
                if entry == "wasserstein_1d" and kind == "f32_3d":
                    continue   # the functional form takes 2-D rows
                out[f"{kind}/{mode}/{entry}"] = _one_case(dev, kind, mode, entry, 100 + k)
    out.update(_hot_cases(dev))
    return out


def main(argv):
    path = argv[1] if len(argv) > 1 else "host_routes.json"
    result = record()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    routes = {}
    for rec in result.values():
        key = " > ".join(rec["names"])
        routes[key] = routes.get(key, 0) + 1
    print(f"{len(result)} cases, {len(routes)} distinct routes -> {path}")


if __name__ == "__main__":
    main(sys.argv)
