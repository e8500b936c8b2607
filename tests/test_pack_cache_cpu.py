"""CPU: the weight-blob cache of scade_amd.run_nerf_helpers.NeRF and the one-launch pack of a train step, with the C
entries replaced by a recorder (no kernels run).

``NeRF.pack(layout)`` must re-pack a blob when a parameter changed in place (``_version``), the raw-pointer epoch
(``ops.PARAM_EPOCH``) moved, a parameter was re-homed, the bf16 flag or the device changed - and not otherwise - and
must re-pack IN PLACE when the blob fits (graph-captured steps hold its address).  ``ops.mlp_pack_step`` must launch
once for the stale networks only and leave what it wrote in their caches; ``ops.StepPacks.tail_args`` must hand the
opening launch the blobs the caches hold."""
import ctypes

import pytest
import torch

from scade_amd import ops
from scade_amd import run_nerf_helpers as H

SIZES = {"scade_mlp_packed_floats": 40, "scade_mlp_packed_t_floats": 48, "scade_mlp_packed_f16_bytes": 96,
         "scade_mlp_packed_t_f16_bytes": 112, "scade_mlp_packed_lp_bytes": 64, "scade_mlp_packed_t_lp_bytes": 72}


class _SizeLib:
    def __getattr__(self, name):
        return lambda: SIZES[name]


def _ptrs(arg, n):
    """the n pointers of a host pointer array the entry received (0 for NULL)"""
    return [p or 0 for p in (ctypes.c_void_p * n).from_address(arg.value)]


@pytest.fixture
def launches(monkeypatch):
    """[(entry, args)] of every C call; the pointer arrays are decoded while they are alive"""
    rec = []

    def call(name, *args):
        if name == "scade_mlp_pack_step":
            n = args[0]
            args = (n, _ptrs(args[1], 24 * n), args[2], _ptrs(args[3], n), _ptrs(args[4], n))
        elif name == "scade_mlp_pack_step_f16x3":
            n = args[0]
            args = (n, _ptrs(args[1], 24 * n), _ptrs(args[2], n), _ptrs(args[3], n), _ptrs(args[4], n))
        elif name.startswith("scade_mlp_pack"):
            args = (_ptrs(args[0], 24),) + args[1:]
        rec.append((name, args))

    monkeypatch.setattr(ops, "call", call)
    monkeypatch.setattr(ops, "stream", lambda: None)
    monkeypatch.setattr(ops, "check", lambda t, what, dtype=torch.float32: t)
    monkeypatch.setattr(ops._lib, "load", lambda: _SizeLib())
    return rec


def _net(seed=0):
    torch.manual_seed(seed)
    return H.NeRF(D=8, W=256, input_ch=57, output_ch=5, skips=[4], input_ch_views=3, input_ch_cam=0, use_viewdirs=True)


@pytest.mark.parametrize("layout", list(ops.PACK_LAYOUTS))
def test_pack_repacks_in_place_exactly_when_the_parameter_state_changes(launches, monkeypatch, layout):
    net = _net()
    bf16 = True if ops.PACK_LAYOUTS[layout].flag else None
    spec = ops.PACK_LAYOUTS[layout]
    blob = net.pack(layout, bf16)
    assert [n for n, _ in launches] == [spec.entry]
    assert blob.numel() == SIZES[spec.size] and blob.dtype == spec.dtype
    assert launches[0][1][0] == [p.data_ptr() for p in net.ordered_params()]
    assert launches[0][1][1].value == blob.data_ptr()
    if spec.flag:
        assert launches[0][1][2] == 1

    def repacked(change):
        del launches[:]
        change()
        got = net.pack(layout, bf16)
        assert got is net.pack(layout, bf16)                   # up to date again: no second pack
        return [n for n, _ in launches]

    assert repacked(lambda: None) == []
    with torch.no_grad():
        assert repacked(lambda: net.pts_linears[3].bias.add_(1.0)) == [spec.entry]       # _version
    monkeypatch.setattr(ops, "PARAM_EPOCH", ops.PARAM_EPOCH + 1)
    assert repacked(lambda: None) == [spec.entry]                                        # raw-pointer epoch
    old = net.feature_linear.weight.data

    def rehome():
        net.feature_linear.weight.data = old.clone()
    assert repacked(rehome) == [spec.entry]                                              # parameter storage
    assert net.pack(layout, bf16).data_ptr() == blob.data_ptr()                          # ... all in place
    if spec.flag:
        bf16 = False
        assert repacked(lambda: None) == [spec.entry] and launches[0][1][2] == 0          # bf16 flag
        assert net.pack(layout, bf16).data_ptr() == blob.data_ptr()
    # a blob on another device (or of another size) is not packed into: a fresh one is allocated
    key = net._packs[layout][1]
    net.adopt(layout, torch.empty(SIZES[spec.size], dtype=spec.dtype, device="meta"), key)
    assert repacked(lambda: None) == [spec.entry]
    assert net.pack(layout, bf16).device.type == "cpu"
    net.adopt(layout, torch.empty(3, dtype=spec.dtype), ())
    assert repacked(lambda: None) == [spec.entry]
    assert net.pack(layout, bf16).numel() == SIZES[spec.size]


def test_the_accessors_are_the_cache(launches):
    net = _net()
    assert net.packed() is net.pack("f32") and net.packed_t() is net.pack("f32_t")
    assert net.packed_f16() is net.pack("f16x3") and net.packed_t_f16() is net.pack("f16x3_t")
    assert net.packed_lp(True) is net.pack("lp", True) and net.packed_t_lp(False) is net.pack("lp_t", False)
    assert len(launches) == 6
    # ... and so are the blobs' earlier attribute names
    assert net._packed is net.pack("f32") and net._packed_t is net.pack("f32_t")
    assert net._packed_f16 is net.pack("f16x3") and net._packed_t_f16 is net.pack("f16x3_t")
    assert net._packed_lp is net.pack("lp", True) and net._packed_t_lp is net.pack("lp_t", False)
    assert _net()._packed is None


def test_the_stand_alone_packs_check_shapes_and_out(launches):
    net = _net()
    ps = list(net.ordered_params())
    for fn in (ops.mlp_pack, ops.mlp_pack_t, ops.mlp_pack_f16, ops.mlp_pack_t_f16):
        with pytest.raises(ValueError):
            fn(ps[:23])
        with pytest.raises(ValueError):
            fn(ps[:3] + [ps[3][:-1]] + ps[4:])
    with pytest.raises(ValueError):
        ops.mlp_pack_lp(ps, True, out=torch.empty(5, dtype=torch.uint8))
    assert launches == []


@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16", "f16x3"])
def test_pack_step_launches_once_for_the_stale_networks_and_adopts_the_blobs(launches, fmt):
    tf = ops.TRAIN_FORMATS[fmt]
    layouts = [l for l in tf.slots if l is not None]
    coarse, fine = _net(1), _net(2)
    entry = "scade_mlp_pack_step_f16x3" if fmt == "f16x3" else "scade_mlp_pack_step"
    blob_args = lambda args: args[2:] if fmt == "f16x3" else args[3:]

    ops.mlp_pack_step([coarse, fine], fmt)
    assert [n for n, _ in launches] == [entry]
    args = launches[0][1]
    assert args[0] == 2 and args[1] == [p.data_ptr() for n in (coarse, fine) for p in n.ordered_params()]
    if fmt != "f16x3":
        assert args[2] == {"f32": 0, "bf16": 1, "f16": 2}[fmt]
    for l, col in zip(layouts, blob_args(args)):
        assert col == [coarse._packs[l][0].data_ptr(), fine._packs[l][0].data_ptr()]
    # adopted: the cache hands the blobs back without packing them again
    del launches[:]
    for net in (coarse, fine):
        for l in layouts:
            blob = net._packs[l][0]
            assert net.pack(l, tf.bf16) is blob and blob.numel() == SIZES[ops.PACK_LAYOUTS[l].size]
    assert launches == []
    ops.mlp_pack_step([coarse, fine], fmt)
    assert launches == []

    # one network touched -> one launch for that network, into the same blobs
    keep = {(id(n), l): n._packs[l][0] for n in (coarse, fine) for l in layouts}
    with torch.no_grad():
        fine.pts_linears[2].weight.mul_(1.5)
    ops.mlp_pack_step([coarse, fine], fmt)
    assert [n for n, _ in launches] == [entry]
    args = launches[0][1]
    assert args[0] == 1 and args[1] == [p.data_ptr() for p in fine.ordered_params()]
    for l, col in zip(layouts, blob_args(args)):
        assert col == [fine._packs[l][0].data_ptr()]
    assert all(n._packs[l][0] is keep[(id(n), l)] for n in (coarse, fine) for l in layouts)
    assert not any(fine.stale(l, ops.layout_key(l, fine.pack_key(), tf.bf16)) for l in layouts)

    # one layout stale -> only that blob is packed (NULL for the others)
    del launches[:]
    del coarse._packs[layouts[-1]]
    ops.mlp_pack_step([coarse, fine], fmt)
    args = launches[0][1]
    cols = blob_args(args)
    assert args[0] == 1 and all(c == [0] for c in cols[:-1]) and cols[-1] == [coarse._packs[layouts[-1]][0].data_ptr()]


@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16", "f16x3"])
def test_step_packs_hand_over_the_cached_blobs(launches, fmt):
    coarse, fine = _net(1), _net(2)
    packs = ops.StepPacks([coarse, fine], fmt)
    with pytest.raises(RuntimeError):
        packs.tail_args()
    packs.prepare()
    assert len(launches) == 1
    code, n, plist, ex, fw, tr = packs.tail_args()
    assert code == {"f32": 0, "bf16": 1, "f16": 2, "f16x3": 3}[fmt] and n == 2
    assert _ptrs(plist, 48) == [p.data_ptr() for net in (coarse, fine) for p in net.ordered_params()]
    for arg, l in zip((ex, fw, tr), ops.TRAIN_FORMATS[fmt].slots):
        assert _ptrs(arg, 2) == ([0, 0] if l is None else [net._packs[l][0].data_ptr() for net in (coarse, fine)])
