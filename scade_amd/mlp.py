"""autograd wrappers of the fused NeRF MLP kernels (scade_mlp_fwd / scade_mlp_bwd)."""
from __future__ import annotations

import torch

from . import ops


def _forward(net, train, inp, viewdirs, bb):
    """-> (out, saved rows or None): ``net``'s forward on x [P,60] (``viewdirs`` None) or pts [N,S,3]; ``train``: in
    its training precision, saving the rows its backward reads (else exact fp32)."""
    if not train:
        return ops.mlp_fwd_net(net, ops.TRAIN_FORMATS["f32"], inp, viewdirs, bb), None
    tf = ops.train_format(net)
    acts = ops.mlp_acts(tf, inp.numel() // inp.shape[-1], inp.device)
    return ops.mlp_fwd_net(net, tf, inp, viewdirs, bb, acts), acts


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
