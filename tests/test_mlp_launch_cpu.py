"""CPU: the launch layer of the NeRF MLP (ops.py's forward / backward launchers and their callers in mlp.py, mlp_bwd.py
and NeRF), with the C entries replaced by a recorder (no kernels run).

Every path a step takes - the forward on x [P,60] and on points, with and without saved rows, the single-network
backward and the joint coarse + fine backward (plain, deferred reduce, first-network hook, precomputed loss-scale maxima,
mismatched 16-bit point tiles, mixed precisions) - is run for every train and inference precision.  The entries it calls,
their arguments (pointers mapped back to named tensors, host pointer arrays decoded) and the KERNEL_TIMER brackets are
compared with ``golden/mlp_launches.json``, recorded from the launch code before it was table-driven.

Regenerate the golden file (only when a launch is meant to change): ``python tests/test_mlp_launch_cpu.py --write``."""
import ctypes
import json
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from scade_amd import mlp, mlp_bwd, ops  # noqa: E402
from scade_amd import run_nerf_helpers as H  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden", "mlp_launches.json")

# made-up sizes, distinct per query so that a buffer sized by the wrong query shows up in the record
SIZES = {
    "scade_mlp_packed_floats": lambda: 40, "scade_mlp_packed_t_floats": lambda: 48,
    "scade_mlp_packed_f16_bytes": lambda: 96, "scade_mlp_packed_t_f16_bytes": lambda: 112,
    "scade_mlp_packed_lp_bytes": lambda: 64, "scade_mlp_packed_t_lp_bytes": lambda: 72,
    "scade_mlp_acts_floats": lambda P: 7 * P + 3, "scade_mlp_acts_lp_bytes": lambda P: 5 * P + 11,
    "scade_mlp_bwd_workspace_floats": lambda P: 2 * P + 1, "scade_mlp_bwd2_workspace_floats": lambda P, Q: 3 * P + Q + 1,
    "scade_mlp_bwd_lp_workspace_bytes": lambda P: 4 * P + 2,
    "scade_mlp_bwd_lp2_workspace_bytes": lambda P, Q: 5 * P + 2 * Q + 3,
    "scade_mlp_lp_point_tiles": lambda P: 2 if P < 16 else 4,
}

# argument kinds per entry: p device pointer, P / I host array of two pointers / ints, D reduce descriptor, v value,
# x not recorded (the 24 parameter pointers of a pack), s stream
KINDS = {
    "scade_mlp_pack": "xps", "scade_mlp_pack_t": "xps", "scade_mlp_pack_f16": "xps", "scade_mlp_pack_t_f16": "xps",
    "scade_mlp_pack_lp": "xpvs", "scade_mlp_pack_t_lp": "xpvs",
    "scade_mlp_fwd": "pvppvpvvpps", "scade_mlp_fwd_f16": "pvppvpvvpps", "scade_mlp_fwd_lp": "pvvppvpvvpps",
    "scade_mlp_bwd": "ppppvpps", "scade_mlp_bwd_f16": "ppppvvpps", "scade_mlp_bwd_lp": "ppvppvpps",
    "scade_mlp_bwd2": "PPPPIPPs", "scade_mlp_bwd2_phases": "PPPPIPPvs", "scade_mlp_bwd2_deferred": "PPPPIPDs",
    "scade_mlp_bwd_f16_2": "PPPPIvPPs", "scade_mlp_bwd_f16_2_deferred": "PPPPIPDs",
    "scade_mlp_bwd_lp2": "PvPPIPPs", "scade_mlp_bwd_lp2_phases": "PvPPIPPvs", "scade_mlp_bwd_lp2_deferred": "PvPPIPPPDs",
}


class _Lib:
    def __getattr__(self, name):
        return SIZES[name]


def _value(a):
    return None if a is None else (a.value or 0 if isinstance(a, ctypes.c_void_p) else a)


def _decode(kind, a):
    if kind == "p" or kind == "D":
        return ("ptr", _value(a))
    if kind == "P":
        return None if a is None else [("ptr", p or 0) for p in (ctypes.c_void_p * 2).from_address(a.value)]
    if kind == "I":
        return list((ctypes.c_int * 2).from_address(a.value))
    return int(a) if isinstance(a, bool) else a


class _Timer:
    def __init__(self, rec):
        self.rec = rec

    def start(self):
        self.rec.append(["timer.start"])
        return object()

    def stop(self, name, t0, work):
        self.rec.append(["timer.stop", name, work])


class _Torch:
    """``torch`` for ops.py: every tensor ops.py allocates is kept alive (no address is reused within a scenario) and
    findable by address (the record names it by size and dtype)"""

    def __init__(self, allocs):
        self.allocs = allocs

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *a, **k):
        t = torch.empty(*a, **k)
        self.allocs[t.data_ptr()] = t
        return t


class Recorder:
    def __init__(self, mp):
        self.rec, self.allocs, self.names, self.keep = [], {}, {}, []
        self.gmax_left = []                       # len(ops.GMAX_READY) after every flush_deferred

        def call(name, *args):
            kinds = KINDS[name]
            assert len(kinds) == len(args), name
            self.rec.append([name, [_decode(k, a) for k, a in zip(kinds, args) if k not in "xs"]])

        mp.setattr(ops, "call", call)
        mp.setattr(ops, "stream", lambda: None)
        mp.setattr(ops, "check", lambda t, what, dtype=torch.float32: t)
        mp.setattr(ops._lib, "load", lambda: _Lib())
        mp.setattr(ops, "torch", _Torch(self.allocs))
        mp.setattr(ops, "KERNEL_TIMER", _Timer(self.rec))
        mp.setattr(ops, "GMAX_READY", {})

    def name(self, **tensors):
        for k, t in tensors.items():
            self.names[t.data_ptr()] = k
            self.keep.append(t)                   # (an address named must not be reused)

    def labelled(self):
        """the record with every pointer replaced by the name of its tensor, or new<k>:<numel>:<dtype> for what the
        launch code allocated (numbered in order of appearance)"""
        new = {}

        def lab(v):
            if isinstance(v, tuple) and v[0] == "ptr":
                p = v[1]
                if p is None or p == 0:
                    return None
                if p in self.names:
                    return self.names[p]
                if p not in new:
                    t = self.allocs.get(p)
                    new[p] = f"new{len(new)}:" + ("?" if t is None else f"{t.numel()}:{str(t.dtype)[6:]}")
                return new[p]
            if isinstance(v, list):
                return [lab(x) for x in v]
            return v
        return [lab(r) for r in self.rec]


N, S0, S1, S_WIDE = 2, 3, 5, 8
ALL_TRAIN = list(H.NeRF.TRAIN_PRECISIONS)
ALL_INFER = list(H.NeRF.INFERENCE_PRECISIONS)


def _net(seed):
    torch.manual_seed(seed)
    return H.NeRF(D=8, W=256, input_ch=57, output_ch=5, skips=[4], input_ch_views=3, input_ch_cam=0, use_viewdirs=True)


def _inputs(r, S, tag=""):
    torch.manual_seed(S)
    rays = torch.rand(N, 8)
    t = dict(x=torch.rand(N * S, 60), pts=torch.rand(N, S, 3), vd=rays[:, 3:6], bb=torch.rand(4))
    r.name(**{k + tag: v for k, v in t.items()}, **{"rays" + tag: rays})
    return t


def _name_blobs(r, **nets):
    for n, net in nets.items():
        for layout, (blob, _) in net._packs.items():
            r.names[blob.data_ptr()] = f"{n}.{layout}"


def sc_train_forward(r, prec):
    net = _net(0)
    net.train_precision = prec
    t = _inputs(r, S0)
    out_x, acts_x = mlp._forward(net, True, t["x"], None, None)
    out_p, acts_p = mlp._forward(net, True, t["pts"], t["vd"], t["bb"])
    r.name(out_x=out_x, acts_x=acts_x, out_p=out_p, acts_p=acts_p)
    _name_blobs(r, net=net)


def sc_infer_forward(r, prec):
    net = _net(0)
    net.inference_precision = prec
    t = _inputs(r, S0)
    with torch.no_grad():
        out_x = net.forward(t["x"])
        out_p = net.forward_points(t["pts"], t["vd"], t["bb"])
    r.name(out_x=out_x, out_p=out_p)
    _name_blobs(r, net=net)


def sc_single_backward(r, prec):
    net = _net(0)
    net.train_precision = prec
    t = _inputs(r, S0)
    _, acts = mlp._forward(net, True, t["pts"], t["vd"], t["bb"])
    del r.rec[:]
    g, sink = torch.rand(N, S0, 4), torch.empty(ops.N_PARAM_FLOATS)
    r.name(acts=acts, g=g, sink=sink)
    flat = mlp_bwd._backward_now(net, acts, g, None)
    r.name(flat=flat)
    assert mlp_bwd._backward_now(net, acts, g, sink) is sink
    _name_blobs(r, net=net)


def _pair(r, prec, order="cf", S_fine=S1, after=False, defer=False, gmax=False, fine_prec=None):
    coarse, fine = _net(1), _net(2)
    coarse.train_precision, fine.train_precision = prec, fine_prec or prec
    items = {}
    for tag, net, S in (("c", coarse, S0), ("f", fine, S_fine)):
        t = _inputs(r, S, tag)
        _, acts = mlp._forward(net, True, t["pts"], t["vd"], t["bb"])
        g, net._grad_sink = torch.rand(N, S, 4), torch.empty(ops.N_PARAM_FLOATS)
        r.name(**{"acts_" + tag: acts, "g_" + tag: g, "sink_" + tag: net._grad_sink})
        items[tag] = (net, acts, g)
        if gmax:
            gm = torch.rand(256)
            ops.GMAX_READY[g.data_ptr()] = gm
            r.name(**{"gmax_" + tag: gm})
    del r.rec[:]
    netname = {id(coarse): "coarse", id(fine): "fine"}
    hook = (lambda net: r.rec.append(["after_net", netname[id(net)]])) if after else None
    ret = mlp_bwd.flush_deferred([items[k] for k in order], hook, defer)
    r.gmax_left.append(len(ops.GMAX_READY))
    if ret is None:
        r.rec.append(["return", None])
    else:
        desc, nets = ret
        r.names[ctypes.addressof(desc.buf)] = "desc"
        r.rec.append(["return", "desc", [netname[id(n)] for n in nets]])
    _name_blobs(r, coarse=coarse, fine=fine)


PAIRS = {
    "pair": dict(), "pair_rev": dict(order="fc"), "pair_defer": dict(defer=True),
    "pair_after": dict(order="fc", after=True), "pair_after_defer": dict(after=True, defer=True),
    "pair_gmax": dict(gmax=True), "pair_gmax_defer": dict(gmax=True, defer=True),
    "pair_gmax_after": dict(gmax=True, after=True), "pair_tiles": dict(S_fine=S_WIDE, gmax=True),
    "pair_tiles_defer": dict(S_fine=S_WIDE, defer=True),
}

SCENARIOS = {}
for _p in ALL_TRAIN:
    SCENARIOS[f"train_forward/{_p}"] = (sc_train_forward, _p, {})
    SCENARIOS[f"single_backward/{_p}"] = (sc_single_backward, _p, {})
    for _k, _kw in PAIRS.items():
        SCENARIOS[f"{_k}/{_p}"] = (_pair, _p, _kw)
for _p in ALL_INFER:
    SCENARIOS[f"infer_forward/{_p}"] = (sc_infer_forward, _p, {})
SCENARIOS["pair_mixed/f32+bf16"] = (_pair, "f32", dict(fine_prec="bf16", gmax=True))
SCENARIOS["pair_mixed_after/f32+f16x3"] = (_pair, "f32", dict(fine_prec="f16x3", after=True))


def run(name):
    fn, prec, kw = SCENARIOS[name]
    with pytest.MonkeyPatch.context() as mp:
        r = Recorder(mp)
        fn(r, prec, **kw)
        return r.labelled(), r.gmax_left


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_launch_sequence_is_pinned(name):
    got, _ = run(name)
    assert json.loads(json.dumps(got)) == _golden()[name]


def test_golden_covers_every_scenario():
    assert sorted(_golden()) == sorted(SCENARIOS)


@pytest.mark.parametrize("name", [n for n in SCENARIOS if n.startswith("pair")])
def test_gmax_ready_does_not_outlive_the_flush(name):
    _, left = run(name)
    assert left == [0]


def test_timer_labels_and_work():
    P0, P1 = N * S0, N * S1
    F = ops.MLP_FLOP_PER_POINT
    seq, _ = run("train_forward/f32")
    assert [r for r in seq if r[0] == "timer.stop"] == [["timer.stop", "mlp_fwd_kernel", P0 * F]]
    for prec, label in (("f16x3", "mlp_fwd_f16_kernel"), ("f16", "mlp_fwd_lp_kernel"), ("bf16", "mlp_fwd_lp_kernel")):
        seq, _ = run(f"infer_forward/{prec}")
        assert [r for r in seq if r[0] == "timer.stop"] == [["timer.stop", label, P0 * F]]
    for prec in ALL_TRAIN:
        seq, _ = run(f"single_backward/{prec}")
        assert [r for r in seq if r[0] == "timer.stop"] == [["timer.stop", "mlp_bwd", 2 * P0 * F]] * 2
        seq, _ = run(f"pair/{prec}")
        # (the exact weight gradient on f16x3 blobs has no joint launch: one backward per network)
        want = [2 * P0 * F, 2 * P1 * F] if prec == "f16x3-dgrad" else [2 * (P0 + P1) * F]
        assert [r for r in seq if r[0] == "timer.stop"] == [["timer.stop", "mlp_bwd", w] for w in want]


FAMILIES = {
    "f32": lambda blob, inp, vd, bb, acts=None: (ops.mlp_fwd_embedded(blob, inp, acts) if vd is None
                                                 else ops.mlp_fwd_points(blob, inp, vd, bb, acts)),
    "f16x3": lambda blob, *a, acts=None: ops.mlp_fwd_f16(blob, *a, acts=acts),
    "lp": lambda blob, *a, acts=None: ops.mlp_fwd_lp(blob, 1, *a, acts=acts),
}
ACTS = {"f32": ("scade_mlp_acts_floats", torch.float32), "f16x3": ("scade_mlp_acts_floats", torch.float32),
        "lp": ("scade_mlp_acts_lp_bytes", torch.uint8)}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_bad_inputs_raise_before_any_launch(family):
    fwd = FAMILIES[family]
    pts, vd, bb = torch.rand(N, S0, 3), torch.rand(N, 3), torch.rand(4)
    size, dtype = ACTS[family]
    short = torch.empty(SIZES[size](N * S0) - 1, dtype=dtype)
    bad = [(pts[..., :2], vd, bb, None), (pts[0], vd, bb, None), (pts, vd[:1], bb, None), (pts, vd[:, :2], bb, None),
           (pts, vd, bb[:3], None), (pts, vd, bb, short)]
    with pytest.MonkeyPatch.context() as mp:
        r = Recorder(mp)
        blob = torch.empty(8)
        for p, v, b, acts in bad:
            with pytest.raises(ValueError):
                fwd(blob, p, v, b, acts=acts)
        x = torch.rand(N * S0, 60)
        with pytest.raises(ValueError):
            fwd(blob, x[:, :59], None, None)
        with pytest.raises(ValueError):
            fwd(blob, x, None, None, acts=short)
        assert r.rec == []
        # exactly the size the query asks for is enough (a slice of a larger buffer, as test_gpu_lp.py passes)
        fwd(blob, pts, vd, bb, acts=torch.empty(SIZES[size](N * S0) + 5, dtype=dtype)[:SIZES[size](N * S0)])
        assert len([c for c in r.rec if c[0].startswith("scade_")]) == 1


@pytest.mark.parametrize("prec", ALL_TRAIN)
def test_single_backward_goes_through_the_public_entry(prec):
    """A step's single-network backward calls ops.mlp_bwd / mlp_bwd_f16 / mlp_bwd_lp by name, so what replaces one of
    them (the GPU tests capture the step's gradients that way) sees the step's backward."""
    name = {"f32": "mlp_bwd", "f16x3": "mlp_bwd_f16", "f16x3-dgrad": "mlp_bwd_f16"}.get(prec, "mlp_bwd_lp")
    seen = []
    with pytest.MonkeyPatch.context() as mp:
        Recorder(mp)
        orig = getattr(ops, name)

        def spy(*a, **k):
            seen.append(k)
            return orig(*a, **k)
        mp.setattr(ops, name, spy)
        net = _net(0)
        net.train_precision = prec
        acts, g = torch.empty(8), torch.rand(N, S0, 4)
        flat = mlp_bwd._backward_now(net, acts, g, None)
    assert len(seen) == 1 and seen[0]["acts"] is acts and seen[0]["g_out"] is g and flat.numel() == ops.N_PARAM_FLOATS
    tf = ops.TRAIN_FORMATS[prec]
    assert seen[0].get("code") == tf.code and seen[0].get("wgrad_f16") == tf.rows24


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    with open(GOLDEN, "w") as f:
        json.dump({n: run(n)[0] for n in SCENARIOS}, f, indent=0, sort_keys=True)
        f.write("\n")
