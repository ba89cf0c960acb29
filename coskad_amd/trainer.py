"""Explicit (autograd-free) train step of STSE on the HIP path: forward, one-class head, backward,
regulariser, Adam -- the reference's `training_step` + optimizer step
(models/euclidean_encoder_dynamicCenter.py:105-122, models/hyperbolic_encoder.py:137-172, Adam at :196)
as a fixed sequence of C-ABI calls on flat parameter / gradient buffers.

Data parallelism (reference: Lightning DDPStrategy, train_COSKAD.py:78): one process per GPU, clips
sharded over ranks, ONE all-reduce of the flat fp32 gradient buffer per step over RCCL, centre statistics
all-reduced when the centre is refreshed.  BatchNorm statistics stay per rank (reference semantics: no
sync_batchnorm).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
import torch.distributed as dist

from . import engine, ops, parallel
from .models.graph_layers.stsgcn import layer_tensors

Tensor = torch.Tensor


class FlatParams:
    """Re-home a module's parameters as views of one flat fp32 buffer (+ a flat gradient buffer),
    in named_parameters() order.  state_dict keys and shapes are untouched."""

    def __init__(self, module: torch.nn.Module) -> None:
        named = [(n, p) for n, p in module.named_parameters()]
        self.names = [n for n, _ in named]
        # every tensor starts on a 16-byte boundary (the layout-specialised kernels load weights as float4); the padding floats
        # stay 0 in the parameter, gradient and Adam buffers
        al = lambda k: (k + 3) // 4 * 4
        total = sum(al(p.numel()) for _, p in named)
        dev = named[0][1].device
        self.flat = torch.zeros(total, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(total, device=dev, dtype=torch.float32)
        # regulariser mask: calc_reg_loss skips tensors whose NAME contains 'bias' (model_utils.py:92)
        self.reg_mask = torch.zeros(total, device=dev, dtype=torch.float32)
        self.views: Dict[str, Tensor] = {}
        self.gviews: Dict[str, Tensor] = {}
        self.n_reg_tensors = 0
        self.offsets: Dict[str, int] = {}
        off = 0
        for n, p in named:
            k = p.numel()
            self.offsets[n] = off
            self.flat[off:off + k].copy_(p.detach().reshape(-1))
            p.data = self.flat[off:off + k].view(p.shape)
            p.grad = self.grad[off:off + k].view(p.shape)
            self.views[n], self.gviews[n] = p.data, p.grad
            if 'bias' not in n:
                self.reg_mask[off:off + k] = 1.0
                self.n_reg_tensors += 1
            off += al(k)


def inv_cov_from_moments(gram: Tensor, acc: Tensor, mu: Tensor, L: int) -> Tensor:
    """inverse of sum (z-mu)(z-mu)^T / (n-1), written with gram = sum z z^T, s = acc[1..L] = sum z, n = acc[Lp+1] (Lp = max(L, 16):
    acc[17] at L <= 16)."""
    s, n = acc[1:1 + L].double(), acc[ops.head_count_slot(L)].double()
    m = mu.double()
    S = gram.double() - torch.outer(m, s) - torch.outer(s, m) + n * torch.outer(m, m)
    return torch.inverse((S / (n - 1)).float())


# the kernels' vocabulary for one ST_GCNN layer's tensors -> the state_dict suffix behind the layer's prefix (`encoder.model.3.`)
_LAYER_NAMES = {"A": "gcn.A", "T": "gcn.T", "Wt": "tcn.0.weight", "bt": "tcn.0.bias", "gt": "tcn.1.weight", "bet": "tcn.1.bias",
                "Wr": "residual.0.weight", "br": "residual.0.bias", "gr": "residual.1.weight", "ber": "residual.1.bias",
                "slope": "prelu.weight"}


def _layer_grad_views(fp: "FlatParams", prefix: str) -> Dict[str, Tensor]:
    """gradient views of one ST_GCNN layer (state_dict prefix `encoder.model.3.`) in the kernels' vocabulary"""
    return {k: fp.gviews[prefix + n] for k, n in _LAYER_NAMES.items() if prefix + n in fp.gviews}


# layers with <= 4 output channels behind 16 / 32 / 64 input channels (the decoder's last layer) run by commutation: both 1x1
# convolutions first, as one streaming pass over the wide input, then mixing / BatchNorm / PReLU on 2 C_out-channel tensors
# (csrc/last_layer.hip).  Tests flip it to hold the two paths against each other.
NARROW_OUT = True


def _is_narrow(m) -> bool:
    return (NARROW_OUT and m.out_channels <= 4 and not m.is_wide and not isinstance(m.residual, torch.nn.Identity)
            and ops.narrow_conv_ok(m.in_channels, 2 * m.out_channels, m.time_dim * m.joints_dim))


# Layers with fewer output than input channels (32 -> 16 on the 25-joint layout) by commutation as well, on their own kernels
# (csrc/commute_layer.hip): convolutions first, mixing / BatchNorm statistics / both adjoints / dA, dT on 16 channels.
COMMUTE = True
COMMUTE_NEXT = True      # ... and the statistics pass of the layer behind them rides on their last kernel


def _is_commute(m, decoder: bool = False) -> bool:
    """decoder: the layer sits in a decoder stack.  At 17 joints the encoder's chained kernels (apply + next statistics, backward +
    reductions of the layer below) already hold a 32 -> 16 layer on chip and the commuted form costs the chain more than it saves; the
    decoder's 32 -> 16 layer stands alone between the folded first layer and the narrow last one (a statistics pass, an apply, a
    reduction pass and a backward kernel of its own), and there the commuted kernels win."""
    tb, rb = m.tcn[1], (m.residual[1] if not isinstance(m.residual, torch.nn.Identity) else None)
    if m.joints_dim == 17 and not decoder:
        return False
    return (COMMUTE and not m.is_wide and rb is not None and ops.commute_ok(m.time_dim, m.joints_dim, m.in_channels, m.out_channels)
            and all(b.momentum is not None and b.affine and b.track_running_stats for b in (tb, rb)) and tb.eps == rb.eps
            and tb.momentum == rb.momentum)


def _virtual_narrow_layer(mod, fp: "FlatParams", prefix: str):
    """The (2 C_out -> C_out) layer that remains behind the commuted convolutions: input [Y; R] = [Wt X; Wr X], `tcn` convolution =
    selector of the Y channels (+ the real bias), `residual` convolution = selector of the R channels (+ the real bias); mixing
    parameters, BatchNorms and PReLU are the real layer's.  -> (LayerTensors, gradient views: the selectors' go to scratch)."""
    from .models.graph_layers.stsgcn import check_bn
    Co, J = mod.out_channels, 2 * mod.out_channels
    tc, tb, rc, rb = mod.tcn[0], mod.tcn[1], mod.residual[0], mod.residual[1]
    check_bn(tb, rb)
    sel = torch.eye(J, device=mod.gcn.A.device).view(J, J, 1, 1)
    sel_t, sel_r = sel[:Co].contiguous(), sel[Co:].contiguous()
    lt = engine.LayerTensors(A=mod.gcn.A, T=mod.gcn.T, Wt=sel_t, bt=tc.bias, gt=tb.weight, bet=tb.bias, rm_t=tb.running_mean,
                             rv_t=tb.running_var, nbt_t=tb.num_batches_tracked, Wr=sel_r, br=rc.bias, gr=rb.weight, ber=rb.bias,
                             rm_r=rb.running_mean, rv_r=rb.running_var, nbt_r=rb.num_batches_tracked, slope=mod.prelu.weight,
                             momentum=tb.momentum if tb.momentum is not None else 0.1, bn=tb if tb.momentum is None else None, cache={})
    return lt, dict(_layer_grad_views(fp, prefix), Wt=torch.empty_like(sel_t), Wr=torch.empty_like(sel_r))


class _Segment:
    """What the segments of a _FlatStack share: `kind`; forward(h, slope, ws, ...) -> (h, slope, saved) with h a pre-activation whose
    PReLU weight is `slope`, or activated (slope None); backward(saved, d, ws, need_dx, in_slope_grad, ...) -> d; `out_slope_grad`, the
    gradient view of the PReLU weight of the segment's LAST layer (written by whoever back-propagates through that PReLU: the segment
    behind, or the stack's caller), None where the segment hands over an activated output.  `in_slope_grad` is the `out_slope_grad` of
    the segment in front (the caller's for the first one); a segment uses it iff its forward consumed a pre-activation."""

    def __getitem__(self, i: int) -> str:
        return (self.kind,)[i]         # seg[0] reads the kind, as it did while segments were tuples


class _TileRun(_Segment):
    """a run of layers the LDS tile kernels take: engine.chain_forward / chain_backward"""
    kind = 'tile'

    def __init__(self, modules, fp: "FlatParams", prefixes, side=None, sync=None) -> None:
        self.layers = [layer_tensors(m) for m in modules]
        self.grads = [_layer_grad_views(fp, p) for p in prefixes]
        self.side, self.sync = side, sync             # engine.SideStream for dA / dT; SyncBN process group
        self.first_layer, self.out_slope_grad = self.layers[0], self.grads[-1]["slope"]

    def forward(self, h, slope, ws, pending0=None):
        """saved: the run's ChainCtx"""
        u, ctx = engine.chain_forward(h, self.layers, True, ws, in_slope=slope, want_ctx=True, sync=self.sync, pending0=pending0)
        return u, self.layers[-1].slope, ctx

    def backward(self, ctx, d, ws, need_dx, in_slope_grad, stats_in=None):
        return engine.chain_backward(ctx, self.layers, d, ws, self.grads, need_dx=need_dx, side=self.side, stats_in=stats_in,
                                     in_slope_grad=in_slope_grad)


def _window_layer(m) -> bool:
    """what every layer on the stored-Z kernels of window length 8 / 16 / 24 needs: that window length, <= 64 channels, no dropout,
    BatchNorms the shared statistics kernel can serve (layer_tensors checks them)"""
    from .models.graph_layers.stsgcn import WIDE_CHANNELS
    if max(m.in_channels, m.out_channels) > WIDE_CHANNELS or m.dropout > 0 or not ops.window_ok(m.time_dim, m.joints_dim):
        return False
    try:
        layer_tensors(m)
    except NotImplementedError:
        return False
    return True


def _is_window(m) -> bool:
    """a layer that is `is_wide` ONLY because of its window length (8 / 16 / 24) and that the stored-Z training kernels take at that
    length"""
    return _window_layer(m) and ops.layer_train_window_ok(m.time_dim, m.joints_dim, m.in_channels, m.out_channels)


def _is_narrow_window(m) -> bool:
    """a (C -> 2) layer of window length 8 / 16 / 24 that runs by commutation like its 12-frame sibling (_is_narrow): the convolutions
    first (csrc/last_layer.hip), then the virtual (4 -> 2) layer on the few-channel stored-Z kernels of that window length
    (ops.layer_train_window_narrow_ok)"""
    T, V = m.time_dim, m.joints_dim
    return (NARROW_OUT and m.out_channels <= 2 and not isinstance(m.residual, torch.nn.Identity) and _window_layer(m)
            and ops.narrow_conv_ok(m.in_channels, 2 * m.out_channels, T * V)
            and ops.layer_train_window_narrow_ok(T, V, 2 * m.out_channels, m.out_channels))


class _WindowRun(_TileRun):
    """a run of layers of window length 8 / 16 / 24 on the stored-Z layer kernels (csrc/train_window_*.hip): the same
    engine.chain_forward / chain_backward calls, whose C-ABI entry points take the geometry; main stream, no SyncBN.  Hands over a
    pre-activation plus its slope, like a tile run."""
    kind = 'window'

    def __init__(self, modules, fp: "FlatParams", prefixes) -> None:
        super().__init__(modules, fp, prefixes, side=None, sync=None)


class _WideLayer(_Segment):
    """a layer beyond the tile kernels on its composed path (stsgcn.wide_forward / wide_backward); hands over an activated output"""
    kind = 'wide'
    out_slope_grad = None

    def __init__(self, mod, fp: "FlatParams", prefix: str) -> None:
        self.mod = mod
        # wide_backward's destinations, by state_dict suffix: the kernels write straight into the flat gradient buffer's views; conv
        # biases in front of a train-mode BatchNorm keep the exact 0 the buffer was created with (nothing ever writes them)
        self.into = {_LAYER_NAMES[k]: g for k, g in _layer_grad_views(fp, prefix).items()}

    def forward(self, h, slope, ws):
        from .models.graph_layers.stsgcn import wide_forward
        xin = ops.prelu_fwd(h, slope) if slope is not None else h
        out, wsaved, wmeta = wide_forward(xin, *self.mod.wide_args())
        return out, None, (wsaved, wmeta, h if slope is not None else None, slope)

    def backward(self, saved, d, ws, need_dx, in_slope_grad):
        from .models.graph_layers.stsgcn import wide_backward
        wsaved, wmeta, pre_u, pre_slope = saved
        res = wide_backward(wsaved, wmeta, d, need_dx=need_dx, into=self.into)
        for n, g in zip(_LAYER_NAMES.values(), res[1:]):
            if g is not None and g.data_ptr() != self.into[n].data_ptr():      # (eval-statistics layers: bias sums)
                self.into[n].copy_(g.view_as(self.into[n]))
        d = res[0] if need_dx else None
        if d is not None and pre_u is not None:       # the layer consumed PReLU(pre_u): back through it, into the producer's slope
            d = ops.prelu_bwd(pre_u, d.contiguous(), pre_slope, in_slope_grad)
        return d


class _CommuteLayer(_Segment):
    """a layer with fewer output than input channels on csrc/commute_layer.hip.  Its last forward kernel can form the first-layer
    statistics of a tile run behind it (`next_layer` -> `pending`, chain_forward's pending0) and its backward kernel the batch
    reductions of a tile run in front (`below` -> `chained`, chain_backward's stats_in); _FlatStack pairs them up."""
    kind = 'commute'

    def __init__(self, mod, fp: "FlatParams", prefix: str) -> None:
        self.mod = mod
        g = _layer_grad_views(fp, prefix)
        self.into = {k: g[k] for k in ("A", "T", "Wt", "Wr", "gt", "bet", "gr", "ber")}
        self.out_slope_grad = g["slope"]

    def forward(self, h, slope, ws, next_layer: Optional[engine.LayerTensors] = None):
        """-> (h, slope, saved, pending)"""
        mod = self.mod
        tc, tb, rc, rb = mod.tcn[0], mod.tcn[1], mod.residual[0], mod.residual[1]
        u, sv, pend = ops.commute_fwd(h, slope, tc.weight, rc.weight, mod.gcn.A, mod.gcn.T, tb.weight, tb.bias, rb.weight, rb.bias,
                                      tc.bias, rc.bias, tb.running_mean, tb.running_var, rb.running_mean, rb.running_var,
                                      tb.num_batches_tracked, rb.num_batches_tracked, tb.momentum, tb.eps,
                                      next_layer=(next_layer.A, next_layer.T) if next_layer is not None else None,
                                      slope_out=mod.prelu.weight)
        return u, mod.prelu.weight, (sv, slope is not None), pend

    def backward(self, saved, d, ws, need_dx, in_slope_grad, below=None):
        """-> (d, chained)"""
        sv, pre_act = saved
        into = self.into
        if pre_act:
            if in_slope_grad is None:
                raise RuntimeError("commuted layer: nowhere to put the gradient of its input's PReLU weight")
            into = dict(into, in_slope=in_slope_grad)
        d, chained = ops.commute_bwd(sv, d.contiguous(), into, below=below)
        return (d if need_dx else None), chained


class _NarrowLayer(_Segment):
    """a layer with <= 4 output channels: both convolutions first, as one streaming pass over the wide input (csrc/last_layer.hip),
    then the few-channel tile kernels on the virtual (2 C_out -> C_out) layer behind them"""
    kind = 'narrow'

    def __init__(self, mod, fp: "FlatParams", prefix: str) -> None:
        self.mod = mod
        self.virt, self.vgrads = _virtual_narrow_layer(mod, fp, prefix)
        g = _layer_grad_views(fp, prefix)
        self.gWt, self.gWr, self.out_slope_grad = g["Wt"], g["Wr"], g["slope"]

    def forward(self, h, slope, ws):
        mod = self.mod
        Co, Ci = mod.out_channels, mod.in_channels
        W4 = torch.cat([mod.tcn[0].weight.view(Co, Ci), mod.residual[0].weight.view(Co, Ci)], 0)
        YR = ops.narrow_conv_fwd(h, slope, W4)                         # [Wt X; Wr X] with X = PReLU(h)
        u, ctx = engine.chain_forward(YR, [self.virt], True, ws, want_ctx=True)
        return u, self.virt.slope, (ctx, h, slope, W4)

    def backward(self, saved, d, ws, need_dx, in_slope_grad):
        ctx, pre_u, pre_slope, W4 = saved
        Co, Ci = self.mod.out_channels, self.mod.in_channels
        dYR = engine.chain_backward(ctx, [self.virt], d, ws, [self.vgrads], need_dx=True)
        d, sums = ops.narrow_conv_bwd(pre_u, pre_slope, W4, dYR)
        self.gWt.copy_(sums[:Co * Ci].view(Co, Ci, 1, 1))
        self.gWr.copy_(sums[Co * Ci:2 * Co * Ci].view(Co, Ci, 1, 1))
        if pre_slope is not None and in_slope_grad is not None:
            in_slope_grad.copy_(sums[2 * Co * Ci:])
        return d if need_dx else None


class _FlatStack:
    """A stack of ST_GCNN layers (Encoder / Decoder `model`, components.py:70-105,143-179) on flat parameter / gradient
    buffers: runs of layers the LDS tile kernels take go through engine.chain_forward / chain_backward (no autograd);
    a layer beyond them (`is_wide`: 64 input channels on the 25-joint layout, > 64 channels, dropout) runs its composed
    HIP path (stsgcn.wide_forward / wide_backward: explicit forward and backward, no autograd), gradients written to the flat
    buffer's views; layers the commuted / narrow-output kernels take run there."""

    def __init__(self, modules, fp: "FlatParams", prefix: str, first: int = 0, plain: bool = False, side=None, sync=None,
                 window: bool = False) -> None:
        """modules: the layers first, first + 1, .. of the nn.Sequential whose parameters are named `{prefix}{index}.`
        plain: no commuted / narrow-output segments (those layers stay in the tile runs); side, sync: the tile runs' side stream /
        SyncBN process group; window: layers of window length 8 / 16 / 24 run on the stored-Z layer kernels where those are built
        (`window` runs) instead of the composed path"""
        kinds = self.kinds(modules, prefix, plain=plain, window=window)
        single = {'wide': _WideLayer, 'narrow': _NarrowLayer, 'commute': _CommuteLayer}
        self.segs = []
        i, n = 0, len(modules)
        while i < n:
            j = i + 1
            if kinds[i] == 'tile':
                while j < n and kinds[j] == 'tile':
                    j += 1
                self.segs.append(_TileRun(modules[i:j], fp, [f"{prefix}{first + k}." for k in range(i, j)], side=side, sync=sync))
            elif kinds[i] == 'window':
                while j < n and kinds[j] == 'window':
                    j += 1
                self.segs.append(_WindowRun(modules[i:j], fp, [f"{prefix}{first + k}." for k in range(i, j)]))
            else:
                self.segs.append(single[kinds[i]](modules[i], fp, f"{prefix}{first + i}."))
            i = j
        self.last_slope_grad = self.segs[-1].out_slope_grad

    @staticmethod
    def kinds(modules, prefix: str, plain: bool = False, window: bool = False) -> List[str]:
        """the segment kind of every layer, as the constructor cuts the stack (needs no parameters' buffers and no device)"""
        dec = prefix.startswith("decoder")

        def beyond(m) -> str:          # an `is_wide` layer: at a window length the stored-Z kernels where asked for and built
            if window and _is_window(m):
                return 'window'
            return 'narrow' if window and not plain and _is_narrow_window(m) else 'wide'

        return [beyond(m) if m.is_wide else 'narrow' if not plain and _is_narrow(m) else
                'commute' if not plain and _is_commute(m, dec) else 'tile' for m in modules]

    def _stats_rider(self, k: int) -> Optional[engine.LayerTensors]:
        """the first layer of a tile run behind commuted segment k when its statistics pass rides on that segment's last kernel"""
        if not (COMMUTE_NEXT and k + 1 < len(self.segs) and self.segs[k + 1].kind == 'tile'):
            return None
        mod, nxt = self.segs[k].mod, self.segs[k + 1].first_layer
        # (25 joints: at 17 the tile kernels' own 16-channel statistics pass is the faster one -- 2.746 vs 2.754 ms on the VAE step)
        if nxt.Ci != mod.out_channels or nxt.rm_t is None or not engine.STORE_Z or mod.joints_dim != 25:
            return None
        return nxt

    def _reductions_rider(self, k: int, saved):
        """(input, Z) of a tile run in front of commuted segment k that is one 2 -> 32 layer fed by the network input: its batch
        reductions ride on that segment's backward kernel"""
        if not (COMMUTE_NEXT and k > 0 and self.segs[k - 1].kind == 'tile'):
            return None
        layers, bctx = self.segs[k - 1].layers, saved[k - 1]
        bl = layers[-1]
        if (bl.Ci == 2 and bl.Co == 32 and bl.Wr is not None and len(layers) == 1 and bctx.in_slope is None
                and bctx.zs and bctx.zs[-1] is not None and bctx.sync is None):
            return bctx.inputs[-1], bctx.zs[-1]
        return None

    def forward(self, x: Tensor, ws: engine.Workspace, in_slope: Optional[Tensor] = None):
        """x: the stack's input, activated (in_slope None) or a pre-activation whose PReLU weight is `in_slope`
        -> (h, slope, saved): apply PReLU(slope) to h for the stack's output (slope None: done)."""
        h, slope, saved = x, in_slope, []
        pend = None                    # the next tile run's first-layer statistics, when the commuted layer in front of it formed them
        for k, seg in enumerate(self.segs):
            if seg.kind == 'commute':
                h, slope, sv, pend = seg.forward(h, slope, ws, next_layer=self._stats_rider(k))
            elif seg.kind == 'tile':
                h, slope, sv = seg.forward(h, slope, ws, pending0=pend)
                pend = None
            else:
                h, slope, sv = seg.forward(h, slope, ws)
            saved.append(sv)
        return h, slope, saved

    def top(self, saved):
        """(ChainCtx, layers) of the last segment when it is a tile run (engine.btlnk_backward), else (None, None)"""
        return (saved[-1], self.segs[-1].layers) if self.segs[-1].kind == 'tile' else (None, None)

    def backward(self, saved, d_last: Tensor, ws: engine.Workspace, need_dx: bool, top_stats=None,
                 in_slope_grad: Optional[Tensor] = None) -> Optional[Tensor]:
        """d_last: gradient w.r.t. the last segment's output (pre-activation U of a tile run -- the caller owns its slope
        gradient -- or the activated output of a wide layer); top_stats: the last tile run's top-layer batch reductions when
        the producer of d_last formed them (engine.btlnk_backward); in_slope_grad: where the gradient of forward's `in_slope`
        goes (the returned gradient is then w.r.t. the PRE-activation input)."""
        d, chained = d_last, None                # batch reductions of the tile run below, formed by the commuted layer's backward kernel
        last = len(self.segs) - 1
        for k in range(last, -1, -1):
            seg = self.segs[k]
            args = (saved[k], d, ws, need_dx or k > 0, self.segs[k - 1].out_slope_grad if k > 0 else in_slope_grad)
            if seg.kind == 'commute':
                d, chained = seg.backward(*args, below=self._reductions_rider(k, saved))
            elif seg.kind == 'tile':
                d = seg.backward(*args, stats_in=top_stats if k == last else chained)
            else:
                d = seg.backward(*args)
        return d


class _FnCtx:
    """what _PlainGCNLayerFn's forward / backward ask of their autograd context, for calling them without autograd"""

    def save_for_backward(self, *tensors) -> None:
        self.saved_tensors = tensors


class _PlainLayer(_Segment):
    """a plain-GCN layer O = relu(W^T X A'^T + bias) on [B, C, P] (alternative_components.py): one fused forward and one fused
    backward kernel (csrc/plain_gcn.hip) where ops.plain_gcn_ok, the strided-GEMM composition of _PlainGCNLayerFn otherwise; hands
    over an activated output.  `adj`: the static encoder's fixed graph (a buffer: no gradient), None for the learnable adjacency."""
    kind = 'plain'
    out_slope_grad = None

    def __init__(self, mod, fp: "FlatParams", prefix: str, adj: Optional[Tensor] = None) -> None:
        self.mod, self.adj = mod, adj
        gv = fp.gviews
        self.gW, self.gb, self.gAdj = gv[prefix + "gcn.weight"], gv.get(prefix + "gcn.bias"), gv.get(prefix + "gcn.Adj")
        self.fused = ops.plain_gcn_ok(mod.in_channels, mod.out_channels, mod.time_dim * mod.joints_dim)

    def forward(self, h, slope, ws):
        gcn = self.mod.gcn
        learn = self.adj is None
        Ap = ops.softmax_rows(gcn.Adj) if learn else self.adj          # formed once: forward and backward share it
        if self.fused:
            # the narrow-side intermediate: Y (mix first) feeds dW; H (channel product first) feeds only the adjacency gradient
            O, S = ops.plain_gcn_fwd(h, gcn.weight, Ap, gcn.bias, save=learn or self.mod.in_channels <= self.mod.out_channels)
            return O, None, (h, Ap, S, O)
        from .models.common.alternative_components import _PlainGCNLayerFn
        ctx = _FnCtx()
        O = _PlainGCNLayerFn.forward(ctx, h, gcn.weight, Ap, gcn.bias)
        return O, None, (h, Ap, ctx, O)

    def backward(self, saved, d, ws, need_dx, in_slope_grad):
        X, Ap, S, O = saved
        gcn = self.mod.gcn
        learn = self.adj is None
        B, Ci, P = X.shape
        if self.fused:
            dX, D = ops.plain_gcn_bwd(X, S, O, d.contiguous().view_as(O), gcn.weight, Ap, self.gW, self.gb, need_dx=need_dx,
                                      need_da=learn)
            if learn:      # dA'[q, p] = sum over (clip, channel) rows of D[r, q] Src[r, p]
                src = X if Ci <= self.mod.out_channels else S
                dA = ops.gemm_rows_outer(D.view(-1, P), src.view(-1, P), torch.empty(P, P, device=X.device, dtype=torch.float32))
        else:
            from .models.common.alternative_components import _PlainGCNLayerFn
            S.needs_input_grad = (need_dx, True, learn, gcn.bias is not None)
            dX, dW, dA, db = _PlainGCNLayerFn.backward(S, d.contiguous().view_as(O))
            self.gW.copy_(dW)
            if db is not None:
                self.gb.copy_(db)
        if learn:
            ops.softmax_rows_bwd(Ap, dA, out=self.gAdj)
        return dX if need_dx else None


class _PlainGCNStack:
    """EncoderLearnablePlainGCN / EncoderStaticPlainGCN behind _FlatStack's interface: one 'plain' segment per layer, on the
    [B, C, T * V] view of the clips."""
    last_slope_grad = None

    def __init__(self, enc, fp: "FlatParams", prefix: str = "encoder.gcns.") -> None:
        adj = getattr(enc, "Adj", None)              # the static encoder's buffer
        self.segs = [_PlainLayer(l, fp, f"{prefix}{i}.", adj) for i, l in enumerate(enc.gcns)]

    def forward(self, x: Tensor, ws: engine.Workspace, in_slope: Optional[Tensor] = None):
        B, C, T, V = x.shape
        h, saved = x.view(B, C, T * V), []
        for seg in self.segs:
            h, _, sv = seg.forward(h, None, ws)
            saved.append(sv)
        return h.view(B, h.shape[1], T, V), None, saved

    def top(self, saved):
        return None, None

    def backward(self, saved, d_last: Tensor, ws: engine.Workspace, need_dx: bool, top_stats=None,
                 in_slope_grad: Optional[Tensor] = None) -> Optional[Tensor]:
        d = d_last
        for k in range(len(self.segs) - 1, -1, -1):
            d = self.segs[k].backward(saved[k], d, ws, need_dx or k > 0, None)
        return d


def _is_plain_gcn(enc) -> bool:
    from .models.common.alternative_components import _PlainGCNEncoder
    return isinstance(enc, _PlainGCNEncoder)


class _OneClassHead:
    """The one-class heads and their centre / covariance bookkeeping (staticCenter.py:40-46,133-155; hyperbolic_encoder.py:175-183)
    for a step object with `model`, `head`, `pg`, `center_acc`, `gram_acc`."""

    def _head(self, z: Tensor):
        """-> (stats block, d loss / d z) of latents z against the centre; accumulates the centre (and covariance) statistics"""
        m = self.model
        if self.head == 'euclidean':
            return ops.mse_head(z, m.c, acc=self.center_acc)[:2]
        if self.head == 'poincare':
            return ops.poincare_head(z, m.c, acc=self.center_acc)[:2]
        if self.head == 'mahalanobis':
            return ops.mahalanobis_head(z, m.c, m.inv_cov_matrix, acc=self.center_acc, gram=self.gram_acc)[:2]
        raise ValueError(f"unknown head {self.head}")

    def refresh_center(self, eps: float = 1e-3) -> Tensor:
        """c <- statistics accumulated since the last refresh (all-reduced over ranks), then reset them."""
        parallel.allreduce_sum_(self.center_acc, self.pg)
        L = self.model.latent_dim
        # Euclidean and Mahalanobis heads accumulate plain sums (mean centre); only the Poincare head's sums are the gyromidpoint's
        c = ops.center_finalize(self.center_acc, eps, L) if self.head != 'poincare' else ops.midpoint_finalize(self.center_acc, L)
        self.model.c.copy_(c)
        self.center_acc.zero_()
        return self.model.c

    def refresh_inv_cov(self, mu: Tensor, reset: bool = True) -> Tensor:
        """inv_cov_matrix <- inverse(sum_n (z_n - mu)(z_n - mu)^T / (n - 1)) over the latents seen since the last
        reset (staticCenter.py:40-46,133-142), from the accumulated second moments (all-reduced over ranks)."""
        parallel.allreduce_sum_(self.gram_acc, self.pg)
        acc = self.center_acc.clone()
        parallel.allreduce_sum_(acc, self.pg)
        self.model.inv_cov_matrix.copy_(inv_cov_from_moments(self.gram_acc, acc, mu, self.model.latent_dim))
        if reset:
            self.gram_acc.zero_()
        return self.model.inv_cov_matrix


def _stacked_heads(m):
    """the VAE's fc_mean | fc_var as one Linear -> (W, b), mean rows first"""
    return torch.cat([m.fc_mean.weight, m.fc_var.weight], 0), torch.cat([m.fc_mean.bias, m.fc_var.bias], 0)


def _unstack_head_grads(gv: Dict[str, Tensor], L: int, gW: Tensor, gb: Tensor) -> None:
    """the stacked Linear's gradients into the four views of fc_mean (rows < L) and fc_var"""
    gv["fc_mean.weight"].copy_(gW[:L]); gv["fc_var.weight"].copy_(gW[L:])
    gv["fc_mean.bias"].copy_(gb[:L]); gv["fc_var.bias"].copy_(gb[L:])


class _LinearProjector:
    """The bottleneck projector, `btlnk` an nn.Linear (ae.py:97-101), on the encoder's pre-activation output U (PReLU `slope` on load).
    Every form: forward(U, slope) -> (y, saved); backward(saved, dy, U, slope, ctx, top_layers, last_slope_grad) -> (dU, top_stats)
    with (ctx, top_layers) = the encoder's _FlatStack.top and top_stats chain_backward's `stats_in` (engine.btlnk_backward).
    Parameters and gradients stay in the flat buffers."""

    def __init__(self, lin, fp: "FlatParams", ws: engine.Workspace, wname: str = "btlnk.") -> None:
        self.lin, self.ws = lin, ws
        self.gW, self.gb = fp.gviews[wname + "weight"], fp.gviews.get(wname + "bias")

    def forward(self, U: Tensor, slope):
        W = self.lin.weight
        return ops.btlnk_fwd(U, W, self.lin.bias, slope, ws=self.ws), W

    def backward(self, W, dy, U, slope, ctx, top_layers, last_slope_grad):
        return engine.btlnk_backward(ctx, top_layers or [], U, W, dy, slope, self.gW, self.gb, last_slope_grad, self.ws)

    def forward_parts(self, U: Tensor, slope):
        """forward without the launch that sums the split-K partials -> (partials, saved): head_backward's input"""
        W = self.lin.weight
        return ops.btlnk_fwd_parts(U, W, slope), W

    def head_backward(self, W, part, c, acc, U, slope, ctx, top_layers, last_slope_grad):
        """the Euclidean head against centre c and `backward` from the partials in one pass -> (stats, dU, top_stats)"""
        return engine.btlnk_head_backward(ctx, top_layers, U, W, part, self.lin.bias, c, slope, self.gW, self.gb, last_slope_grad,
                                          self.ws, acc=acc)


class _MLPProjector(_LinearProjector):
    """`mlp` projector (components.py:209-226): the wide first Linear on the bottleneck kernel, then every [BatchNorm1d, ReLU, Linear]
    block on csrc/mlp_head.hip"""

    def __init__(self, mlp, fp: "FlatParams", ws: engine.Workspace) -> None:
        super().__init__(mlp.net[0], fp, ws, "btlnk.net.0.")
        gv = fp.gviews
        self.blocks = [(bn, lin, {"gamma": gv[f"btlnk.net.{3 * i + 1}.weight"], "beta": gv[f"btlnk.net.{3 * i + 1}.bias"],
                                  "W2": gv[f"btlnk.net.{3 * i + 3}.weight"], "b2": gv.get(f"btlnk.net.{3 * i + 3}.bias")})
                       for i, (bn, lin) in enumerate(mlp.blocks())]

    def forward(self, U: Tensor, slope):
        if U.shape[0] == 1:                # nn.BatchNorm1d's own check in training mode
            raise ValueError("Expected more than 1 value per channel when training (BatchNorm1d of the mlp projector)")
        y, W = super().forward(U, slope)
        saved = []
        for bn, lin, _ in self.blocks:
            z, stat = ops.mlp_head_fwd(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                       lin.weight, lin.bias, True, momentum=ops.bn_momentum(bn), eps=bn.eps)
            saved.append((y, stat))
            y = z
        return y, (W, saved)

    def backward(self, saved, dy, *top):
        W, block_saved = saved
        for (bn, lin, g), (y_in, stat) in zip(reversed(self.blocks), reversed(block_saved)):
            dy = ops.mlp_head_bwd(y_in, stat, bn.weight, bn.bias, lin.weight, dy, g, True)
        return super().backward(W, dy, *top)


class _StackedHeads:
    """the VAE's mean | concentration heads on the encoder's output (`btlnk` is Identity): their weights stacked, one pass over U"""

    def __init__(self, model, fp: "FlatParams", ws: engine.Workspace) -> None:
        self.model, self.ws, self.gv = model, ws, fp.gviews

    def forward(self, U: Tensor, slope):
        W, b = _stacked_heads(self.model)
        return ops.btlnk_fwd(U, W, b, slope, ws=self.ws), (W, b)

    def backward(self, saved, dy, U, slope, ctx, top_layers, last_slope_grad):
        W, b = saved
        gW, gb = torch.empty_like(W), torch.empty_like(b)
        res = engine.btlnk_backward(ctx, top_layers or [], U, W, dy, slope, gW, gb, last_slope_grad, self.ws)
        _unstack_head_grads(self.gv, self.model.latent_dim, gW, gb)
        return res


def _projector(model, fp: "FlatParams", ws: engine.Workspace):
    """the projector form of a model the step classes admitted"""
    from .models.common.components import MLP
    if isinstance(model.btlnk, MLP):
        return _MLPProjector(model.btlnk, fp, ws)
    if isinstance(model.btlnk, torch.nn.Linear):
        return _LinearProjector(model.btlnk, fp, ws)
    return _StackedHeads(model, fp, ws)


def _check_clip(val, algorithm):
    """(clip value, 0.0 = off; algorithm) of the keywords grad_clip_val / grad_clip_algorithm, Lightning's gradient_clip_val /
    gradient_clip_algorithm (None: 'norm')"""
    import math
    val = 0.0 if val is None else float(val)
    algorithm = 'norm' if algorithm is None else str(algorithm)
    if not math.isfinite(val) or val < 0:
        raise ValueError(f"grad_clip_val must be finite and >= 0 (0 / None: off), got {val}")
    if algorithm not in ops.CLIP_MODES:
        raise ValueError(f"grad_clip_algorithm {algorithm!r}: 'norm' or 'value'")
    return val, algorithm


def _check_accumulate(k) -> int:
    if k is None:
        return 1
    if int(k) != k or int(k) < 1:
        raise ValueError(f"accumulate must be a whole number >= 1, got {k!r}")
    return int(k)


class _FlatStep:
    """What the autograd-free steps share: the model's parameters re-homed in flat buffers, the bottleneck projector, Adam's moments and
    the fused update, the regulariser, the data-parallel world."""

    use_graph = False

    def __init__(self, model, lr: float, alpha: float, betas, eps: float, process_group, grad_clip_val=0.0,
                 grad_clip_algorithm: str = 'norm', accumulate: int = 1) -> None:
        """grad_clip_val, grad_clip_algorithm, accumulate: Lightning's gradient_clip_val / gradient_clip_algorithm /
        accumulate_grad_batches (0 / None: no clipping; 1: an update per step)"""
        self.accumulate = _check_accumulate(accumulate)
        self.clip_val, self.clip_mode = _check_clip(grad_clip_val, grad_clip_algorithm)
        self.model, self.alpha, self.lr = model, float(alpha), float(lr)
        self.beta1, self.beta2, self.eps = float(betas[0]), float(betas[1]), float(eps)
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        self.fp = FlatParams(model)
        self.m, self.v = torch.zeros_like(self.fp.flat), torch.zeros_like(self.fp.flat)
        self.ws = engine.Workspace()
        self.projector = _projector(model, self.fp, self.ws)
        self.reg_scale = 0.5 / self.fp.n_reg_tensors          # calc_reg_loss value = reg_scale * sum p^2
        self.reg_coef = self.alpha * 2.0 * self.reg_scale      # its gradient coefficient, times alpha
        self.steps = 0
        self.updates = 0                   # optimiser updates so far (= steps unless gradients accumulate)
        # gradient accumulation: the backward kernels overwrite fp.grad, so every micro-step adds it into `acc`; `_micro` counts the
        # micro-steps of the pending group
        self.acc = torch.zeros_like(self.fp.grad) if self.accumulate > 1 else None
        self._micro = 0
        dev = self.fp.flat.device
        self.clip_partials = torch.zeros(ops.CLIP_PARTIALS, device=dev, dtype=torch.float64)
        self.last_grad_norm = torch.zeros(1, device=dev, dtype=torch.float32)       # unclipped norm of the last update (norm mode)

    def set_lr(self, lr: float) -> None:
        self.lr = float(lr)

    def set_gradient_clip(self, val, algorithm: Optional[str] = None) -> None:
        """change the clip value (0 / None: off), and the algorithm when given, between steps"""
        val, mode = _check_clip(val, self.clip_mode if algorithm is None else algorithm)
        if self.use_graph and getattr(self, "_graph", None) is not None and (val, mode) != (self.clip_val, self.clip_mode):
            raise ValueError("use_graph: the captured step holds the clip value as a launch argument; set it before the first step")
        self.clip_val, self.clip_mode = val, mode

    def reg_loss(self) -> Tensor:
        """utils/model_utils.py::calc_reg_loss value of the current parameters (1-element tensor)."""
        return ops.sqnorm(self.fp.flat, self.fp.reg_mask, self.reg_scale)

    def _adam(self, grad: Optional[Tensor] = None, gscale: Optional[float] = None, reg_coef: Optional[float] = None) -> None:
        """torch.optim.Adam step on the flat buffers with alpha * calc_reg_loss' gradient and the 1 / world of the gradient
        all-reduce folded in.  Outside hipGraph capture lr and the running products beta^t come from the host (one launch);
        a captured step keeps them in device memory (`hyper`: a one-thread launch advances beta^t in front of the update).
        grad, gscale, reg_coef: another gradient buffer, its scale and the regulariser's coefficient (the accumulated one's).
        With clipping on, the update runs on the
        clipping forms of the same two kernels; by norm, one launch in front of them leaves the squared norm's partials."""
        g = self.fp.grad if grad is None else grad
        gscale = 1.0 / self.world if gscale is None else gscale
        reg_coef = self.reg_coef if reg_coef is None else reg_coef
        fp, clip = self.fp, self.clip_val > 0
        if clip and self.clip_mode == 'norm':
            ops.grad_sqnorm(g, fp.flat, fp.reg_mask, gscale, reg_coef, partials=self.clip_partials)
        if self.use_graph:
            if clip:
                ops.adam_clip_dev(fp.flat, g, self.m, self.v, fp.reg_mask, self.hyper, self.beta1, self.beta2, self.eps,
                                  self.clip_partials, self.clip_val, self.clip_mode, self.last_grad_norm, gscale=gscale,
                                  reg_coef=reg_coef)
            else:
                ops.adam_dev(fp.flat, g, self.m, self.v, fp.reg_mask, self.hyper, self.beta1,
                             self.beta2, self.eps, gscale=gscale, reg_coef=reg_coef)
            return
        import numpy as np
        b1p, b2p = getattr(self, "_bpow", (np.float32(1.0), np.float32(1.0)))
        self._bpow = (np.float32(b1p * np.float32(self.beta1)), np.float32(b2p * np.float32(self.beta2)))   # fp32, as the device tick
        self.updates += 1
        if clip:
            ops.adam_clip_pow(fp.flat, g, self.m, self.v, fp.reg_mask, self.lr, self.beta1, self.beta2, self.eps,
                              float(self._bpow[0]), float(self._bpow[1]), self.clip_partials, self.clip_val, self.clip_mode,
                              self.last_grad_norm, gscale=gscale, reg_coef=reg_coef)
        else:
            ops.adam_pow(fp.flat, g, self.m, self.v, fp.reg_mask, self.lr, self.beta1, self.beta2, self.eps,
                         float(self._bpow[0]), float(self._bpow[1]), gscale=gscale, reg_coef=reg_coef)

    def _micro_step(self) -> None:
        """accumulate > 1, after a backward: fp.grad joins the group's sum; the group's last micro-step updates"""
        ops.grad_accum(self.acc, self.fp.grad, first=self._micro == 0)
        self._micro += 1
        if self._micro == self.accumulate:
            self.flush()

    def flush(self) -> bool:
        """Apply a pending group of fewer than `accumulate` micro-steps (Lightning steps on the last batch of an epoch whatever its
        index), each still counting 1 / accumulate -> whether an update was made.  The regulariser is part of every micro-batch's
        loss, so j micro-steps carry j / accumulate of its gradient: all of it for a whole group (the factor is then exactly 1).
        One all-reduce of the accumulated buffer per update; none on the micro-steps before it (Lightning's no_sync)."""
        if self._micro == 0:
            return False
        if self.world > 1:
            dist.all_reduce(self.acc, group=self.pg)
        self._adam(self.acc, 1.0 / (self.world * self.accumulate), self.reg_coef * (self._micro / self.accumulate))
        self._micro = 0
        return True

    def _update(self) -> None:
        """after a backward that left this rank's gradient in fp.grad, all of it at once"""
        if self.accumulate > 1:
            return self._micro_step()
        if self.world > 1:
            dist.all_reduce(self.fp.grad, group=self.pg)                          # SUM; the 1 / W is folded into Adam
        self._adam()

    # -- optimiser state in torch.optim.Adam's layout -------------------------------------------------------------------------
    def _beta_pows(self):
        import numpy as np
        if self.use_graph:
            h = self.hyper.detach().cpu().numpy()
            return np.float32(h[1]), np.float32(h[2])
        return getattr(self, "_bpow", (np.float32(1.0), np.float32(1.0)))

    def state_dict(self) -> dict:
        """torch.optim.Adam's state_dict of this step (per parameter in named_parameters() order: step, exp_avg, exp_avg_sq as copies
        of the flat moments' views; one param group), loadable into torch.optim.Adam(model.parameters()); beside it, under 'coskad',
        what a bit-exact continuation needs and torch does not keep: the fp32 running products beta^t and the micro-step counter."""
        fp = self.fp
        updates = self.steps if self.use_graph else self.updates
        state = {}
        if updates > 0:
            for i, n in enumerate(fp.names):
                off, shape = fp.offsets[n], fp.views[n].shape
                k = fp.views[n].numel()
                state[i] = {'step': torch.tensor(float(updates)), 'exp_avg': self.m[off:off + k].view(shape).clone(),
                            'exp_avg_sq': self.v[off:off + k].view(shape).clone()}
        group = {'lr': self.lr, 'betas': (self.beta1, self.beta2), 'eps': self.eps, 'weight_decay': 0, 'amsgrad': False,
                 'params': list(range(len(fp.names)))}
        b1p, b2p = self._beta_pows()
        return {'state': state, 'param_groups': [group],
                'coskad': {'beta_pows': (float(b1p), float(b2p)), 'micro_step': self._micro, 'updates': updates,
                           'last_grad_norm': float(self.last_grad_norm)}}

    def load_state_dict(self, sd: dict) -> None:
        """state_dict()'s inverse, in place into the flat moments; takes torch.optim.Adam's state_dict of the same parameters too (the
        running products are then multiplied up in fp32, step by step, as this step would have)."""
        import numpy as np
        fp = self.fp
        groups = sd['param_groups']
        if len(groups) != 1 or len(groups[0]['params']) != len(fp.names):
            raise ValueError(f"optimizer state: expected one param group of {len(fp.names)} parameters")
        g = groups[0]
        if g.get('amsgrad') or g.get('weight_decay') or g.get('maximize'):
            raise ValueError("optimizer state: the fused Adam has no amsgrad, weight_decay or maximize")
        own = sd.get('coskad', {})
        if own.get('micro_step', 0):
            raise ValueError("optimizer state: saved inside an accumulation group (mid-epoch checkpoints are not supported)")
        state = sd['state']
        steps = {int(float(s['step'])) for s in state.values()}
        if len(steps) > 1 or (state and len(state) != len(fp.names)):
            raise ValueError("optimizer state: every parameter must carry the same step count")
        updates = steps.pop() if steps else 0
        self.m.zero_(); self.v.zero_()
        for i, n in enumerate(fp.names if state else ()):
            s = state[g['params'][i]]
            off, k = fp.offsets[n], fp.views[n].numel()
            self.m[off:off + k].copy_(s['exp_avg'].reshape(-1))
            self.v[off:off + k].copy_(s['exp_avg_sq'].reshape(-1))
        self.beta1, self.beta2, self.eps = float(g['betas'][0]), float(g['betas'][1]), float(g['eps'])
        self.set_lr(float(g['lr']))
        if 'beta_pows' in own:
            b1p, b2p = (np.float32(b) for b in own['beta_pows'])
        else:
            b1p = b2p = np.float32(1.0)
            for _ in range(updates):
                b1p, b2p = np.float32(b1p * np.float32(self.beta1)), np.float32(b2p * np.float32(self.beta2))
        self._bpow = (b1p, b2p)
        if getattr(self, "hyper", None) is not None:
            self.hyper[1], self.hyper[2] = float(b1p), float(b2p)
        self.updates = self.steps = updates
        self._micro = 0
        self.last_grad_norm.fill_(float(own.get('last_grad_norm', 0.0)))      # (logged before the first update of an epoch)



class STSETrainStep(_FlatStep, _OneClassHead):
    """One-class training of an STSE (`linear` projector, or `mlp` within the HIP kernels' widths) without autograd: the STS-GCN
    encoder, or a plain-GCN encoder (EncoderLearnablePlainGCN / EncoderStaticPlainGCN) on csrc/plain_gcn.hip.

    head: 'euclidean' -> F.mse_loss(z, c);  'poincare' -> dist(c, project(expmap0(z))).mean().
    """

    def __init__(self, model, lr: float = 1e-4, alpha: float = 1e-6, head: str = 'euclidean',
                 betas=(0.9, 0.999), eps: float = 1e-8, process_group=None, use_graph: bool = False,
                 side_stream: bool = False, sync_bn: bool = False, fused_window: bool = False, grad_clip_val=0.0,
                 grad_clip_algorithm: str = 'norm', accumulate: int = 1) -> None:
        """fused_window: encoder layers of window length 8 / 16 / 24 train on the stored-Z layer kernels where those are built
        (`window` runs of the stack; off: the composed path, as before)
        grad_clip_val, grad_clip_algorithm, accumulate: gradient clipping ('norm' | 'value'; 0 / None: off) and accumulation over
        `accumulate` calls of `step` (eager only), as Lightning's Trainer arguments of those meanings"""
        from .models.sts.ae import STSE
        from .models.common.components import MLP
        mlp = isinstance(model.btlnk, MLP)
        if not isinstance(model, STSE) or not (isinstance(model.btlnk, torch.nn.Linear) or (mlp and model.btlnk.hip_ok)):
            raise TypeError("STSETrainStep drives an STSE with projector='linear' or an 'mlp' within the kernels' widths")
        if use_graph and _check_accumulate(accumulate) > 1:
            raise ValueError("use_graph: a captured step makes one update per replay; accumulate > 1 runs eagerly")
        super().__init__(model, lr, alpha, betas, eps, process_group, grad_clip_val, grad_clip_algorithm, accumulate)
        self.head = head
        dev = self.fp.flat.device
        self.hyper = torch.tensor([lr, 1.0, 1.0, 0.0], device=dev, dtype=torch.float32)
        L = model.latent_dim
        self.center_acc = torch.zeros(ops.head_slots(L), device=dev, dtype=torch.float32)
        self.gram_acc = torch.zeros(L, L, device=dev, dtype=torch.float32) if head == 'mahalanobis' else None
        # an encoder with layers beyond the LDS tile kernels (the wide C = 2 -> 256 stack, dropout) runs them on their explicit forward /
        # backward between the tile runs: main stream, eager launches
        plain_gcn = _is_plain_gcn(model.encoder)
        wide = plain_gcn or any(l.is_wide for l in model.encoder.model)
        if plain_gcn and (side_stream or use_graph):
            raise ValueError("a plain-GCN encoder runs on the main stream, outside hipGraph capture")
        if wide and (side_stream or use_graph):
            raise ValueError("an encoder with wide layers runs on the main stream, outside hipGraph capture")
        # optional: dA / dT on a second stream beside the next layer's reductions.  Measured SLOWER on MI355X (2.43 vs
        # 2.28 ms/step: the two LDS-heavy persistent kernels halve each other's occupancy), so it is off by default.
        self.side = engine.SideStream() if side_stream else None
        # optional SyncBN of the encoder's BatchNorm2d layers (the reference's DDP keeps per-rank statistics): every
        # BatchNorm boundary of the forward and the backward adds the other ranks' fp64 sums (engine.chain_forward / _backward)
        self.sync_group = None
        if sync_bn and self.world > 1:
            if mlp or side_stream or use_graph or wide:
                raise ValueError("sync_bn: encoder BatchNorm only (STS-GCN encoder within the tile kernels, linear projector), on the "
                                 "main stream, outside hipGraph capture")
            self.sync_group = process_group if process_group is not None else dist.group.WORLD
        # the commuted kernels take a layer (32 -> 16 on the 25-joint layout) unless the step is asked for something only the plain
        # chain does: hipGraph capture, the side stream, SyncBN; an encoder without wide or commuted layers is one tile run (a
        # narrow-output layer alone does not split it)
        if plain_gcn:
            self.stack = _PlainGCNStack(model.encoder, self.fp)
        else:
            plain = not wide and (use_graph or side_stream or sync_bn or not any(_is_commute(l) for l in model.encoder.model))
            self.stack = _FlatStack(list(model.encoder.model), self.fp, "encoder.model.", plain=plain, side=self.side,
                                    sync=self.sync_group, window=fused_window)
        # gradient buckets for the data-parallel all-reduce: [encoder | bottleneck]; the bottleneck parameters are the
        # tail of the flat buffer (named_parameters order) and their gradients are final before the encoder backward
        names = self.fp.names
        first_tail = next((i for i, n in enumerate(names) if n.startswith("btlnk.")), None)
        tail = first_tail is not None and all(n.startswith("btlnk.") for n in names[first_tail:])
        self.tail_off = self.fp.offsets[names[first_tail]] if tail else None
        if use_graph and any(isinstance(b, torch.nn.modules.batchnorm._BatchNorm) and b.momentum is None for b in model.modules()):
            raise ValueError("use_graph: BatchNorm with momentum=None changes its averaging factor every step (a launch argument here); "
                             "capture needs a fixed momentum")
        self.use_graph = use_graph
        self._graph = self._x_static = self._stats_static = None

    @property
    def layers(self) -> List[engine.LayerTensors]:
        """the encoder's LayerTensors when it is one tile run, else []"""
        segs = self.stack.segs
        return segs[0].layers if len(segs) == 1 and segs[0].kind == 'tile' else []

    def set_lr(self, lr: float) -> None:
        self.hyper[0] = lr                 # the captured step reads it
        self.lr = float(lr)

    # -- the step ---------------------------------------------------------------------------
    def _body(self, x: Tensor) -> Tensor:
        U, slope, saved_stack = self.stack.forward(x, self.ws)          # slope None: the stack ended in a wide layer (activated output)
        ctx, top_layers = self.stack.top(saved_stack)
        if (type(self.projector) is _LinearProjector and self.head == 'euclidean' and self.side is None
                and engine.head_rides(ctx, top_layers or [], U, self.model.latent_dim)):
            # the head rides in the bottleneck backward's launch, which forms dz from the forward's partials (engine.HEAD_RIDES)
            part, saved = self.projector.forward_parts(U, slope)
            stats, dU, top_stats = self.projector.head_backward(saved, part, self.model.c, self.center_acc, U, slope, ctx, top_layers,
                                                                self.stack.last_slope_grad)
        else:
            z, saved = self.projector.forward(U, slope)
            stats, dz = self._head(z)
            # (the side-stream backward runs its own batch reductions: no ChainCtx, so the bottleneck's backward forms none)
            dU, top_stats = self.projector.backward(saved, dz, U, slope, ctx if self.side is None else None, top_layers,
                                                    self.stack.last_slope_grad)
        work = None
        if self.world > 1 and self.tail_off is not None and self.accumulate == 1:
            # bucket 1 (87 % of the bytes: the bottleneck weight) is complete now: its all-reduce runs on the collective
            # stream while the encoder backward proceeds (SUM; the 1/W is folded into Adam)
            work = dist.all_reduce(self.fp.grad[self.tail_off:], group=self.pg, async_op=True)
        self.stack.backward(saved_stack, dU, self.ws, need_dx=False, top_stats=top_stats)
        if self.accumulate > 1:            # no collective inside a group; one all-reduce of the accumulated buffer at its end
            self._micro_step()
            return stats
        if self.world > 1:
            head = self.fp.grad if work is None else self.fp.grad[:self.tail_off]
            dist.all_reduce(head, group=self.pg)           # bucket 2: the encoder's gradients (0.12 MB)
            if work is not None:
                work.wait()
        self._adam()
        return stats

    def step(self, x: Tensor) -> Tensor:
        """One optimisation step on clips x [B,C,T,V]; returns the head's stats block (stats[0] = loss)."""
        self.steps += 1
        x = x.contiguous()
        if not self.use_graph:
            return self._body(x)
        if self._graph is None or self._x_static.shape != x.shape:
            self._x_static = x.clone()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):          # warm-up outside capture (allocator, lazy module load)
                self._body(self._x_static)
            torch.cuda.current_stream().wait_stream(s)
            self.steps += 1
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                self._stats_static = self._body(self._x_static)
        self._x_static.copy_(x)
        self._graph.replay()
        self.updates = self.steps
        ops.note_raw_write()                    # the replay runs the captured writers without their wrappers
        return self._stats_static


class _LatentHead:
    """The latent head of the decoder step, between the projector's output y and the decoder entry's input z_dec.
    forward(y) -> (z_dec, dz0, losses, saved): dz0 the head's own gradient w.r.t. z_dec (None: all of it comes back through the
    decoder), losses the 'head' (and 'exp') entries of the step's result; backward(saved, dz) -> dy."""

    def __init__(self, step: "STSAETrainStep", heads: bool = False) -> None:
        """heads: the VAE's two small head Linears act on y here (`mlp` projector; else the projector stacked them)"""
        self.model, self.acc, self.gv, self.heads = step.model, step.center_acc, step.fp.gviews, heads
        self.beta, self.gamma = step.beta, step.gamma


class _CentreLatent(_LatentHead):
    """the autoencoder's: MSE(z, c) against the centre and its gradient, which the decoder's backward adds to"""

    def forward(self, y: Tensor):
        stats, dz, _ = ops.mse_head(y, self.model.c, acc=self.acc)
        return y, dz, {'head': stats[0:1]}, None

    def backward(self, saved, dz: Tensor) -> Tensor:
        return dz


class _PowerSphericalLatent(_LatentHead):
    """The PowerSpherical head on csrc/vae_head.hip (normalise, softplus + 1, Householder sample, KL, 1 / kappa: three launches +
    torch's Beta draw instead of ~80 element-wise launches under autograd); the two small Linears of the `mlp` projector's heads ride
    on the strided GEMM with the weights stacked"""

    def forward(self, y: Tensor):
        m, L = self.model, self.model.latent_dim
        Wc, H2 = None, y
        if self.heads:
            Wc, bc = _stacked_heads(m)                                        # [L + 1, L]
            H2 = ops.gemm(y, Wc.t(), bias=bc, bias_mode=2)
        zs, kl_rows, ik_rows, ps_saved = ops.ps_head_forward(H2[:, :L], H2[:, L:L + 1])
        return zs, None, {'head': kl_rows.mean().reshape(1), 'exp': ik_rows.mean().reshape(1)}, (y, H2, Wc, ps_saved)

    def backward(self, saved, dz: Tensor) -> Tensor:
        y, H2, Wc, ps_saved = saved
        L, B = self.model.latent_dim, dz.shape[0]
        dH2 = torch.empty_like(H2)
        ops.ps_head_backward(ps_saved, dz, self.beta / B, self.gamma / B, dH2[:, :L], dH2[:, L:L + 1])
        if Wc is None:
            return dH2
        # the two heads' Linears (weights stacked): dWc = dH2^T y, db = column sums, dy = dH2 Wc
        dWc = ops.gemm_rows_outer(dH2, y.contiguous(), torch.empty(L + 1, L, device=dH2.device, dtype=torch.float32))
        _unstack_head_grads(self.gv, L, dWc, dH2.sum(0))
        return ops.gemm(dH2, Wc)


class _GaussianLatent(_LatentHead):
    """The Gaussian head (`distribution: 'normal'`) on csrc/vae_head_normal.hip: softplus + 1, the reparameterised sample, KL to the
    standard normal and 1 / sigma in one launch on torch's normal draw, their backward in another -- instead of the element-wise
    launches of _AutogradLatent and its autograd graph; the two small Linears of the `mlp` projector's heads ride on the strided GEMM
    with the weights stacked ([2L, L]), as in _PowerSphericalLatent"""

    def __init__(self, step: "STSAETrainStep", heads: bool = False) -> None:
        super().__init__(step, heads)
        names = ("fc_mean.weight", "fc_mean.bias", "fc_var.weight", "fc_var.bias") if heads else ()
        self.head_params, self.head_grads = [step.model.get_parameter(n) for n in names], [self.gv[n] for n in names]

    def forward(self, y: Tensor):
        m, L = self.model, self.model.latent_dim
        Wc, H2 = None, y
        if self.heads:
            Wc, bc = _stacked_heads(m)                                        # [2L, L]
            H2 = ops.gemm(y, Wc.t(), bias=bc, bias_mode=2)
        zs, kl_rows, inv_rows, saved = ops.normal_head_forward(H2[:, :L], H2[:, L:])
        losses = {'head': kl_rows.mean().reshape(1), 'exp': (inv_rows.sum() / (y.shape[0] * L)).reshape(1)}
        return zs, None, losses, (y, H2, Wc, saved)

    def backward(self, saved, dz: Tensor) -> Tensor:
        y, H2, Wc, head_saved = saved
        L, B = self.model.latent_dim, dz.shape[0]
        dH2 = torch.empty_like(H2)
        ops.normal_head_backward(head_saved, dz, self.beta / B, self.gamma / (B * L), dH2[:, :L], dH2[:, L:])
        if Wc is None:
            return dH2
        # the two heads' Linears (weights stacked): dWc = dH2^T y, db = column sums, dy = dH2 Wc
        dWc = ops.gemm_rows_outer(dH2, y.contiguous(), torch.empty(2 * L, L, device=dH2.device, dtype=torch.float32))
        _unstack_head_grads(self.gv, L, dWc, dH2.sum(0))
        return ops.gemm(dH2, Wc)


class _AutogradLatent(_LatentHead):
    """every other distribution of the VAE, and the Gaussian head without `gaussian_head` (the yardstick _GaussianLatent is held
    against): torch ops on [B, latent] tensors under a local autograd graph (vae.py:79-91,104-118)"""

    def __init__(self, step: "STSAETrainStep", heads: bool = False) -> None:
        super().__init__(step, heads)
        names = ("fc_mean.weight", "fc_mean.bias", "fc_var.weight", "fc_var.bias") if heads else ()
        self.head_params, self.head_grads = [step.model.get_parameter(n) for n in names], [self.gv[n] for n in names]

    def forward(self, y: Tensor):
        m, L = self.model, self.model.latent_dim
        y.requires_grad_(True)
        with torch.enable_grad():
            if self.heads:
                Z_mean, Z_var = m._finish_heads(m.fc_mean(y), m.fc_var(y), None, False)
            else:
                Z_mean, Z_var = m._finish_heads(y[:, :L], y[:, L:], None, False)
            q, p = m.reparameterize(Z_mean, Z_var)
            zs = q.rsample()
            loss_kl = torch.distributions.kl.kl_divergence(q, p).sum(-1).mean()
            loss_exp = (1 / Z_var).mean()
            small = self.beta * loss_kl + self.gamma * loss_exp
        losses = {'head': loss_kl.detach().reshape(1), 'exp': loss_exp.detach().reshape(1)}
        return zs.detach().contiguous(), None, losses, (y, zs, small)

    def backward(self, saved, dz: Tensor) -> Tensor:
        y, zs, small = saved
        res = torch.autograd.grad([zs, small], [y] + self.head_params, [dz, torch.ones_like(small)])
        for into, g in zip(self.head_grads, res[1:]):
            into.copy_(g)
        return res[0].contiguous()


class _PlainEntry:
    """The decoder entry where the decoder's first layer is not folded into it (else: lowrank.LowRankFirstLayer, the same two calls):
    rev_btlnk (ae.py:223-227), H = z Wr^T + br straight into the decoder's [B, hid, T, V] view; backward dWr = dH^T z, dbr = sum dH,
    dz (+)= dH Wr into the flat gradient views: streaming kernels over H / dH at latent 8 / 16 (csrc/rev_btlnk.hip), three MFMA GEMMs at
    17 .. 512 (csrc/rev_btlnk_wide.hip), the strided GEMM at the other small latents"""

    def __init__(self, model, gviews) -> None:
        self.rev, self.shape = model.rev_btlnk, (model.hidden_dimension, model.n_frames, model.n_joints)
        self.gW, self.gb, self._z = gviews["rev_btlnk.weight"], gviews["rev_btlnk.bias"], None

    def forward(self, z: Tensor) -> Tensor:
        self._z = z
        return ops.rev_btlnk_fwd(z, self.rev.weight, self.rev.bias).view(z.shape[0], *self.shape)

    def backward(self, dH: Tensor, dz: Optional[Tensor] = None) -> Tensor:
        z, self._z = self._z, None
        return ops.rev_btlnk_bwd(dH.reshape(z.shape[0], -1), z, self.rev.weight, self.gW, self.gb, dz=dz)


class STSAETrainStep(_FlatStep):
    """One optimisation step of the decoder models on flat parameter / gradient buffers with the fused Adam -- the
    reference's training_step + optimizer step of

      mode 'ae'  (models/euclidean_autoencoder.py:106-118): lambda_ * MSE(x_rec, x) + MSE(z, c) + alpha * reg
      mode 'vae' (models/spherical_vae.py:81-107):          phi * MSE(x_rec, x) + alpha * reg + beta * KL(q || p) + gamma * mean(1 / kappa)

    encoder stack -> `projector` (the bottleneck, one kernel pass; the VAE's mean | concentration heads stacked) -> `latent` (MSE to
    the centre | the PowerSpherical head | the Gaussian head | another distribution under a local autograd graph) -> `entry` (rev_btlnk,
    with the first decoder layer folded in where lowrank.py takes it) -> decoder stack -> reconstruction head -> the same stages backwards.  The
    constructor picks every stage's form and refuses what they do not take; gradients land in the flat buffer; data-parallel
    all-reduce and Adam as in STSETrainStep."""

    def __init__(self, model, mode: str = 'ae', lr: float = 1e-4, alpha: float = 0.0, lambda_: float = 0.01, phi: float = 1.0,
                 beta: float = 1.0, gamma: float = 1.0, betas=(0.9, 0.999), eps: float = 1e-8, process_group=None,
                 fused_window: bool = False, gaussian_head: bool = False, grad_clip_val=0.0, grad_clip_algorithm: str = 'norm',
                 accumulate: int = 1) -> None:
        """grad_clip_val, grad_clip_algorithm, accumulate: as STSETrainStep's.
        fused_window: layers of window length 8 / 16 / 24 train on the stored-Z layer kernels where those are built (`window` runs
        of both stacks, the last decoder layer as a `narrow` segment; off: the composed path, as before).  Eager, main stream.
        gaussian_head: a `distribution: 'normal'` VAE runs its latent head on csrc/vae_head_normal.hip (_GaussianLatent) where
        `gaussian_head_ok` admits it; off: under the local autograd graph (_AutogradLatent), as before."""
        from .models.sts.ae import STSAE
        from .models.sts.vae import STSVAE
        from .models.common.components import Encoder
        if not isinstance(model, STSAE) or not isinstance(model.encoder, Encoder):
            raise TypeError("STSAETrainStep drives an STSAE / STSVAE with the STS-GCN encoder")
        if mode not in ('ae', 'vae') or (mode == 'vae') != isinstance(model, STSVAE):
            raise ValueError(f"mode {mode!r} does not fit {type(model).__name__}")
        if not self.supports(model):
            raise TypeError("STSAETrainStep: projector / latent size outside the bottleneck, head and decoder-entry kernels ('linear' "
                            f"projector with head rows <= {ops.BTLNK_LMAX}, or an 'mlp' within MLP.hip_ok; not in ops.AE_WIDE_OFF)")
        # a stack ending `wide` hands over an activated output (no slope, no `last_slope_grad`), which neither the bottleneck kernels
        # nor the reconstruction head take: refused before anything touches the model (its parameters are not re-homed yet)
        for kinds, which in zip(self.segment_kinds(model, fused_window), ("an encoder", "a decoder")):
            if kinds[-1] == 'wide':
                raise NotImplementedError(f"STSAETrainStep: {which} ending in a wide layer")
        super().__init__(model, lr, alpha, betas, eps, process_group, grad_clip_val, grad_clip_algorithm, accumulate)
        self.mode = mode
        self.lambda_, self.phi, self.beta, self.gamma = float(lambda_), float(phi), float(beta), float(gamma)
        self.w_rec = self.lambda_ if mode == 'ae' else self.phi
        self.enc = _FlatStack(list(model.encoder.model), self.fp, "encoder.model.", window=fused_window)
        # the decoder's first layer sees a rank-(latent + 1) input (rev_btlnk of the latent): folded into one streaming pass where that
        # layer would otherwise take the composed wide path (coskad_amd/lowrank.py); it then hands over a pre-activation and its slope
        from . import lowrank
        dec_layers, gv = list(model.decoder.model), self.fp.gviews
        self.lowrank = self.entry_slope = self.entry_slope_grad = None
        if self._folds_first(model):
            self.lowrank = self.entry = lowrank.LowRankFirstLayer(model.rev_btlnk, dec_layers[0], gv)
            self.entry_slope, self.entry_slope_grad = dec_layers[0].prelu.weight, gv["decoder.model.0.prelu.weight"]
        else:
            self.entry = _PlainEntry(model, gv)
        first = 0 if self.lowrank is None else 1
        self.dec = _FlatStack(dec_layers[first:], self.fp, "decoder.model.", first=first, window=fused_window)
        self.center_acc = torch.zeros(ops.head_slots(model.latent_dim), device=self.fp.flat.device, dtype=torch.float32)
        latent = _CentreLatent if mode == 'ae' else _PowerSphericalLatent if model.distribution == 'ps' else _AutogradLatent
        if gaussian_head and mode == 'vae' and self.gaussian_head_ok(model):
            latent = _GaussianLatent
        self.latent = latent(self, heads=isinstance(self.projector, _MLPProjector))
        self.last = {}

    @staticmethod
    def supports(model) -> bool:
        """the stages take the model: latents up to 512 -- above 16 on csrc/btlnk_wide.hip, vae_head.hip's wave-per-clip kernels and rev_btlnk_wide.hip
        (the decoder entry is then _PlainEntry), unless a measurement switched that latent off (ops.AE_WIDE_OFF)"""
        from .models.sts.vae import STSVAE
        from .models.common.components import MLP
        L = model.latent_dim
        if L > ops.BTLNK_LMAX or (L > 16 and L in ops.AE_WIDE_OFF):
            return False
        rows = 16 if L <= 16 else ops.BTLNK_LMAX          # a latent within 16 keeps the narrow kernels' rule
        if isinstance(model, STSVAE):
            if isinstance(model.btlnk, MLP):              # `projector: 'mlp'` (spherical_vae.yaml:37): MLP, then the heads on its output
                return model.btlnk.hip_ok and (L > 16 or model.btlnk.hidden_layers[0] <= 16)
            return isinstance(model.btlnk, torch.nn.Identity) and L + model.fc_var.out_features <= rows
        return isinstance(model.btlnk, torch.nn.Linear)

    @staticmethod
    def gaussian_head_ok(model) -> bool:
        """a `distribution: 'normal'` VAE whose latent the Gaussian head's kernels take, unless a measurement switched its
        (projector, latent) off (ops.NORMAL_HEAD_OFF)"""
        from .models.common.components import MLP
        L, proj = model.latent_dim, 'mlp' if isinstance(model.btlnk, MLP) else 'linear'
        return (getattr(model, 'distribution', None) == 'normal' and ops.normal_head_ok(L)
                and not any(p == proj and lo <= L <= hi for p, lo, hi in ops.NORMAL_HEAD_OFF))

    @staticmethod
    def _folds_first(model) -> bool:
        """the decoder's first layer is folded into rev_btlnk's streaming pass (coskad_amd/lowrank.py)"""
        from . import lowrank
        dec_layers = list(model.decoder.model)
        return (len(dec_layers) > 1 and lowrank.LowRankFirstLayer.supports(model.rev_btlnk, dec_layers[0])
                and (lowrank.MODE == 'always' or (lowrank.MODE == 'wide' and dec_layers[0].is_wide)))

    @staticmethod
    def segment_kinds(model, fused_window: bool = False):
        """-> (encoder kinds, decoder kinds behind a folded first layer), one per layer, as the constructor would cut the two stacks; the wrappers ask
        before they build a step (a stack with `wide` segments at a window length stays with them on the autograd route)"""
        dec_layers = list(model.decoder.model)
        first = 1 if STSAETrainStep._folds_first(model) else 0
        return (_FlatStack.kinds(list(model.encoder.model), "encoder.model.", window=fused_window),
                _FlatStack.kinds(dec_layers[first:], "decoder.model.", window=fused_window))

    def step(self, x: Tensor) -> Dict[str, Tensor]:
        """-> {'rec': F.mse_loss(x_rec, x), 'head': MSE(z, c) | KL, ('exp': mean(1 / kappa)), 'z': the latents}"""
        self.steps += 1
        x = x.contiguous()
        U, slope, enc_saved = self.enc.forward(x, self.ws)
        y, proj_saved = self.projector.forward(U, slope)
        z, dz, losses, latent_saved = self.latent.forward(y)
        Ud, slope_d, dec_saved = self.dec.forward(self.entry.forward(z), self.ws, in_slope=self.entry_slope)
        # reconstruction head: PReLU of the last layer + MSE + its gradient in one kernel
        loss_rec, dUd, _ = ops.rec_head(Ud, x, slope_d, dslope=self.dec.last_slope_grad, upstream=self.w_rec)
        out = dict(losses, z=z, rec=loss_rec)
        # ---- backward ----------------------------------------------------------------------------------------------------
        d = self.dec.backward(dec_saved, dUd, self.ws, need_dx=True, in_slope_grad=self.entry_slope_grad)
        dy = self.latent.backward(latent_saved, self.entry.backward(d, dz=dz))
        ctx, top_layers = self.enc.top(enc_saved)
        dU, top_stats = self.projector.backward(proj_saved, dy, U, slope, ctx, top_layers, self.enc.last_slope_grad)
        self.enc.backward(enc_saved, dU, self.ws, need_dx=False, top_stats=top_stats)
        self._update()
        self.last = out
        return out


class AutogradTrainStep(_OneClassHead):
    """Same interface as STSETrainStep for models the flat-buffer path does not take: `mlp` projectors and latents beyond the
    bottleneck kernels' widths; and the plain-GCN encoders when make_train_step is not asked for `flat_plain_gcn` (its default:
    this step is the yardstick the flat plain-GCN step is held against).  Forward / backward go through the module
    surface (autograd nodes around the HIP kernels, library GEMMs where the module uses them); the one-class head and
    its gradient are the HIP head kernels (`z.backward(dz)`), the regulariser gradient is added to `.grad`, the
    optimiser is torch's Adam (calc_reg_loss / configure_optimizers of the reference wrappers)."""

    def __init__(self, model, lr: float = 1e-4, alpha: float = 1e-6, head: str = 'euclidean', betas=(0.9, 0.999),
                 eps: float = 1e-8, process_group=None, grad_clip_val=0.0, grad_clip_algorithm: str = 'norm',
                 accumulate: int = 1) -> None:
        self.model, self.head, self.alpha, self.pg = model, head, float(alpha), process_group
        self.accumulate = _check_accumulate(accumulate)
        self.clip_val, self.clip_mode = _check_clip(grad_clip_val, grad_clip_algorithm)
        self._micro = 0
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        self.params = [(n, p) for n, p in model.named_parameters()]
        self.reg_params = [p for n, p in self.params if 'bias' not in n]          # model_utils.py:92
        self.reg_scale = 0.5 / max(1, len(self.reg_params))
        self.opt = torch.optim.Adam([p for _, p in self.params], lr=lr, betas=betas, eps=eps)
        dev = self.params[0][1].device
        L = model.latent_dim
        self.center_acc = torch.zeros(ops.head_slots(L), device=dev, dtype=torch.float32)
        self.gram_acc = torch.zeros(L, L, device=dev, dtype=torch.float32) if head == 'mahalanobis' else None
        self.steps = 0
        self.last_grad_norm = torch.zeros(1, device=dev, dtype=torch.float32)

    def set_lr(self, lr: float) -> None:
        for g in self.opt.param_groups:
            g['lr'] = lr

    def set_gradient_clip(self, val, algorithm: Optional[str] = None) -> None:
        self.clip_val, self.clip_mode = _check_clip(val, self.clip_mode if algorithm is None else algorithm)

    def step(self, x: Tensor) -> Tensor:
        self.steps += 1
        m = self.model
        if self._micro == 0:               # (no zero_grad inside an accumulation group: autograd sums into .grad)
            self.opt.zero_grad(set_to_none=True)
        z = m(x)
        zd = z.detach().contiguous()
        stats, dz = self._head(zd)
        z.backward(dz if self.accumulate == 1 else dz / self.accumulate)
        with torch.no_grad():
            coef = self.alpha * 2.0 * self.reg_scale / self.accumulate         # d/dp of alpha * reg_scale * sum p^2
            for p in self.reg_params:
                if p.grad is not None:
                    p.grad.add_(p, alpha=coef)
        self._micro += 1
        if self._micro == self.accumulate:
            self.flush()
        return stats

    def flush(self) -> bool:
        """the update of the pending group (every micro-step counted 1 / accumulate), also of fewer than `accumulate` micro-steps
        at the end of an epoch -> whether one was made"""
        if self._micro == 0:
            return False
        _clipped_update([p for _, p in self.params], self.opt, self.pg, self.clip_val, self.clip_mode, self.last_grad_norm)
        self._micro = 0
        return True

    def state_dict(self) -> dict:
        """torch.optim.Adam's state_dict, with the micro-step counter beside it"""
        return dict(self.opt.state_dict(), coskad={'micro_step': self._micro})

    def load_state_dict(self, sd: dict) -> None:
        _load_torch_optimizer(self.opt, sd)
        self._micro = 0

    def reg_loss(self) -> Tensor:
        with torch.no_grad():
            return self.reg_scale * sum((p.float() ** 2).sum() for p in self.reg_params).reshape(1)


def _clipped_update(params, opt, pg, clip_val: float, clip_mode: str, norm_out: Optional[Tensor] = None) -> None:
    """the autograd routes' update: gradient mean over ranks, torch's clipping (after the mean, as on the flat steps), opt.step()"""
    with torch.no_grad():
        parallel.allreduce_grads_mean_(params, pg)   # one flat bucket
    if clip_val > 0:
        if clip_mode == 'norm':
            norm = torch.nn.utils.clip_grad_norm_(params, clip_val)
            if norm_out is not None:
                norm_out.copy_(norm.reshape(1))
        else:
            torch.nn.utils.clip_grad_value_(params, clip_val)
    opt.step()


def _load_torch_optimizer(opt, sd: dict) -> None:
    """a step class' state_dict() -- a flat step's or an autograd route's -- into a torch optimiser, the project key left aside"""
    if sd.get('coskad', {}).get('micro_step', 0):
        raise ValueError("optimizer state: saved inside an accumulation group (mid-epoch checkpoints are not supported)")
    opt.load_state_dict({k: v for k, v in sd.items() if k != 'coskad'})


def make_train_step(model, flat_plain_gcn: bool = False, fused_window: bool = False, **kw):
    """STSETrainStep (flat buffers, fused Adam, no autograd) for every STS-GCN encoder -- tile kernels and wide layers alike -- with a
    linear or in-width mlp projector, and with `flat_plain_gcn` for the plain-GCN encoders (Learnable_GCN / Static_GCN) behind such
    a projector too (fused layer kernels, csrc/plain_gcn.hip; the wrappers ask for it).  AutogradTrainStep for what is left:
    projectors / latents beyond the bottleneck kernels, and the plain-GCN encoders without `flat_plain_gcn`.
    `fused_window`: an STS-GCN encoder of window length 8 / 16 / 24 runs its layers on the stored-Z layer kernels where those are built
    (csrc/train_window_*.hip; the wrappers ask for it) instead of the composed path; still eager, on the main stream."""
    from .models.common.components import MLP, Encoder
    btl, enc = getattr(model, 'btlnk', None), getattr(model, 'encoder', None)
    proj_ok = isinstance(btl, torch.nn.Linear) or (isinstance(btl, MLP) and btl.hip_ok)
    flat = (proj_ok and model.latent_dim <= ops.BTLNK_LMAX
            and (isinstance(enc, Encoder) or (flat_plain_gcn and _is_plain_gcn(enc))))
    if not flat or _is_plain_gcn(enc) or any(l.is_wide for l in enc.model):
        # plain-GCN and wide layers, and the autograd step: main stream, eager launches; the optional key `sync_batchnorm` (absent in
        # the reference): with one rank there is nothing to synchronise
        kw.pop('use_graph', None); kw.pop('side_stream', None)
        if kw.get('sync_bn') and not (dist.is_available() and dist.is_initialized() and dist.get_world_size(kw.get('process_group')) > 1):
            kw.pop('sync_bn')
    if flat:
        return STSETrainStep(model, fused_window=fused_window, **kw)
    if kw.pop('sync_bn', False):
        raise ValueError("sync_bn: encoder BatchNorm only (STS-GCN encoder within the tile kernels, linear projector)")
    return AutogradTrainStep(model, **kw)


def make_decoder_step(model, mode: str, fused_window: bool = True, wide_latent: bool = False, gaussian_head: bool = False,
                      **kw) -> Optional[STSAETrainStep]:
    """STSAETrainStep for an autoencoder / VAE within its kernels, None for what stays on torch autograd + torch.optim.Adam: another
    encoder, a projector / latent outside `supports`, a stack ending in a `wide` segment.  `fused_window` (not a key of the reference's
    yamls): at window length 8 / 16 / 24 the flat step takes the model when the stored-Z layer kernels serve EVERY layer of both stacks
    (no `wide` segment: such a stack -- 8-channel layers, a joint layout without window kernels -- stays on the autograd route, as
    does every model with `fused_window` off).  `wide_latent` (the wrappers ask for it; their yaml key `flat_wide_latent`): a latent
    beyond 16 that `supports` admits takes the flat step too (csrc/vae_head.hip, rev_btlnk_wide.hip); off: the autograd route.
    `gaussian_head` (the wrappers ask for it; their yaml key `flat_gaussian_head`): the step of a `distribution: 'normal'` VAE runs its
    latent head on csrc/vae_head_normal.hip; off: that head stays under its local autograd graph."""
    from .models.common.components import Encoder
    if not isinstance(getattr(model, 'encoder', None), Encoder) or not STSAETrainStep.supports(model):
        return None
    if model.latent_dim > 16 and not wide_latent:
        return None
    window = (fused_window and ops.window_ok(model.n_frames, model.n_joints)
              and not any('wide' in kinds for kinds in STSAETrainStep.segment_kinds(model, fused_window=True)))
    if any(kinds[-1] == 'wide' for kinds in STSAETrainStep.segment_kinds(model, fused_window=window)):
        return None
    return STSAETrainStep(model, mode=mode, fused_window=window, gaussian_head=gaussian_head, **kw)
