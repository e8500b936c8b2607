"""autograd wrappers of the fused NeRF MLP kernels (scade_mlp_fwd / scade_mlp_bwd)."""
from __future__ import annotations

import torch

from . import ops


def _forward(net, train, inp, viewdirs, bb):
    """-> (out, saved rows or None): the kernel and the weight blob of ``net``'s forward on x [P,60] (``viewdirs``
    None) or pts [N,S,3]; ``train``: in its training precision, saving the rows its backward reads."""
    if not train:
        if viewdirs is None:
            return ops.mlp_fwd_embedded(net.packed(), inp), None
        return ops.mlp_fwd_points(net.packed(), inp, viewdirs, bb), None
    tf = ops.TRAIN_FORMATS.get(net.train_precision)
    if tf is None:
        raise ValueError("NeRF.train_precision must be one of %s" % (net.TRAIN_PRECISIONS,))
    P = inp.shape[0] if viewdirs is None else inp.shape[0] * inp.shape[1]
    if tf.code is not None:
        acts = ops.mlp_acts_lp_alloc(P, inp.device)
        return ops.mlp_fwd_lp(net.packed_lp(tf.bf16), tf.code, inp, viewdirs, bb, acts), acts
    acts = ops.mlp_acts_alloc(P, inp.device)
    if tf.step == "f16x3":
        rows24 = net.train_precision == "f16x3"
        return ops.mlp_fwd_f16(net.packed_f16(), inp, viewdirs, bb, acts, rows24=rows24), acts
    if viewdirs is None:
        return ops.mlp_fwd_embedded(net.packed(), inp, acts), acts
    return ops.mlp_fwd_points(net.packed(), inp, viewdirs, bb, acts), acts


class MlpEmbeddedFn(torch.autograd.Function):
    """NeRF.forward(x[P,60])  (model/run_nerf_helpers.py:223-247)."""

    @staticmethod
    def forward(ctx, net, train, x, *params):
        out, acts = _forward(net, train, x, None, None)
        ctx.net, ctx.mode = net, 0
        ctx.save_for_backward(x, acts if acts is not None else x.new_empty(0))
        return out

    @staticmethod
    def backward(ctx, g_out):
        from .mlp_bwd import mlp_backward
        x, acts = ctx.saved_tensors
        grads = mlp_backward(ctx.net, acts, g_out)
        return (None, None, None) + tuple(grads)


class MlpPointsFn(torch.autograd.Function):
    """run_network fused with the positional encoding (run_scade_scannet.py:48-63)."""

    @staticmethod
    def forward(ctx, net, train, pts, viewdirs, bb, *params):
        out, acts = _forward(net, train, pts, viewdirs, bb)
        ctx.net, ctx.mode, ctx.n_params = net, 1, len(params)
        ctx.save_for_backward(pts, viewdirs, bb, acts if acts is not None else pts.new_empty(0))
        return out

    @staticmethod
    def backward(ctx, g_out):
        from .mlp_bwd import mlp_backward
        pts, viewdirs, bb, acts = ctx.saved_tensors
        grads = mlp_backward(ctx.net, acts, g_out)
        if ctx.n_params != len(grads):
            # the forward saw a gradient sink and passed one stand-in parameter (NeRF.forward_points): the sink has
            # taken the gradient and there is nothing to return - unless the sink was detached in between
            if any(g is not None for g in grads):
                raise RuntimeError("scade_amd: the gradient sink of this network was detached between the forward and "
                                   "the backward of a step")
            return (None,) * (5 + ctx.n_params)
        return (None, None, None, None, None) + tuple(grads)
