"""Mirror of the reference's models/common/components.py (Encoder / Decoder / MLP) on the HIP path."""
from __future__ import annotations

from typing import List, Tuple, Union

import torch
import torch.nn as nn

from ... import engine, ops
from ..graph_layers.stsgcn import ST_GCNN_layer, _PReLUFn, run_stack

Tensor = torch.Tensor


class _Stack(nn.Module):
    """nn.Sequential of ST_GCNN layers run as one fused chain."""

    def _build(self, chans: List[int], n_frames: int, n_joints: int, dropout: float, bias: bool) -> None:
        layers = nn.ModuleList()
        for ci, co in zip(chans[:-1], chans[1:]):
            layers.append(ST_GCNN_layer(in_channels=ci, out_channels=co, kernel_size=(1, 1), stride=1,
                                        time_dim=n_frames, joints_dim=n_joints, dropout=dropout, bias=bias))
        self.model = nn.Sequential(*layers)
        self._ws = engine.Workspace()

    def forward_preact(self, X: Tensor) -> Tuple[Tensor, Tensor]:
        """-> (U_last, slope_last): the fused path's hand-over to a consumer that applies PReLU on load."""
        return run_stack(X, list(self.model), self._ws)

    def forward(self, X: Tensor) -> Tensor:
        u, slope = self.forward_preact(X)
        return u if slope is None else _PReLUFn.apply(u, slope)


class Encoder(_Stack):
    """STS-GCN encoder: channels input_dim -> layer_channels... -> hidden_dimension
    (reference components.py:47-105)."""

    def __init__(self, input_dim: int, layer_channels: List[int], hidden_dimension: int, n_frames: int,
                 n_joints: int, dropout: float, bias: bool = True,
                 device: Union[str, torch.device] = 'cpu') -> None:
        super().__init__()
        self.input_dim, self.layer_channels, self.hidden_dimension = input_dim, layer_channels, hidden_dimension
        self.n_frames, self.n_joints, self.dropout, self.bias, self.device = n_frames, n_joints, dropout, bias, device
        self.build_model()

    def build_model(self) -> None:
        self._build([self.input_dim] + list(self.layer_channels) + [self.hidden_dimension],
                    self.n_frames, self.n_joints, self.dropout, self.bias)


class Decoder(_Stack):
    """STS-GCN decoder: hidden_dimension -> reversed(layer_channels)... -> output_dim
    (reference components.py:109-179)."""

    def __init__(self, output_dim: int, layer_channels: List[int], hidden_dimension: int, n_frames: int,
                 n_joints: int, dropout: float, bias: bool = True,
                 device: Union[str, torch.device] = 'cpu') -> None:
        super().__init__()
        self.output_dim, self.layer_channels, self.hidden_dimension = output_dim, list(layer_channels)[::-1], hidden_dimension
        self.n_frames, self.n_joints, self.dropout, self.bias, self.device = n_frames, n_joints, dropout, bias, device
        self.build_model()

    def build_model(self) -> None:
        self._build([self.hidden_dimension] + list(self.layer_channels) + [self.output_dim],
                    self.n_frames, self.n_joints, self.dropout, self.bias)


class _MLPHeadFn(torch.autograd.Function):
    """z = W2 . relu(BatchNorm1d(y1)) + b2 on the HIP kernels of csrc/mlp_head.hip (forward, running-statistics update,
    backward)."""

    @staticmethod
    def forward(ctx, y1, gamma, beta, W2, b2, bn, training):
        y1 = y1.contiguous()
        if training and y1.shape[0] == 1:        # nn.BatchNorm1d's own check (torch/nn/functional.py: _verify_batch_size)
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(y1.shape)}")
        training = ops.bn_batch_stats(bn, training)      # track_running_stats=False: batch statistics in eval mode too
        z, stat = ops.mlp_head_fwd(y1, gamma, beta, bn.running_mean, bn.running_var, bn.num_batches_tracked, W2.contiguous(), b2,
                                   training, momentum=ops.bn_momentum(bn) if training else 0.0, eps=bn.eps)
        ctx.save_for_backward(y1, stat, gamma, beta, W2)
        ctx.training, ctx.has_b2 = training, b2 is not None
        return z

    @staticmethod
    def backward(ctx, dz):
        y1, stat, gamma, beta, W2 = ctx.saved_tensors
        g = {"gamma": torch.empty_like(gamma), "beta": torch.empty_like(beta), "W2": torch.empty_like(W2)}
        if ctx.has_b2:
            g["b2"] = torch.empty(W2.shape[0], device=W2.device, dtype=W2.dtype)
        dy1 = ops.mlp_head_bwd(y1, stat, gamma, beta, W2.contiguous(), dz.contiguous(), g, ctx.training)
        return dy1, g["gamma"], g["beta"], g["W2"], g.get("b2"), None, None


class MLP(nn.Module):
    """[Linear -> BatchNorm1d -> ReLU] per hidden size + final Linear (reference components.py:183-240,
    whose constructor is broken -- SURVEY 8a row a8; this implements the evident intent and accepts both
    `hidden_layers=` and the `hidden_size=` spelling STSE passes at ae.py:161; parity unpinned).

    HIP path (`forward_preact`, taken by STSE / STSVAE): the first, wide Linear runs on the bottleneck kernels with the
    encoder's PReLU fused into the load, every following [BatchNorm1d, ReLU, Linear] block on csrc/mlp_head.hip.
    Widths beyond those kernels (any hidden size or the output > 64) compose torch modules instead."""

    def __init__(self, input_size: int, output_size: int, hidden_layers: List[int] = None, bias=True,
                 device: Union[str, torch.device] = 'cpu', *, hidden_size: List[int] = None) -> None:
        super().__init__()
        hidden_layers = hidden_layers if hidden_layers is not None else hidden_size
        self.input_size, self.output_size, self.hidden_layers, self.bias = input_size, output_size, list(hidden_layers or []), bias
        self.build_model()

    def build_model(self) -> None:
        layer_list, input_size = [], self.input_size
        for next_dim in self.hidden_layers:
            layer_list += [nn.Linear(input_size, next_dim, bias=self.bias), nn.BatchNorm1d(next_dim), nn.ReLU(inplace=True)]
            input_size = next_dim
        layer_list.append(nn.Linear(input_size, self.output_size, bias=self.bias))
        self.net = nn.Sequential(*layer_list)

    @property
    def hip_ok(self) -> bool:
        hs = self.hidden_layers
        # (BatchNorm1d with momentum=None or without running statistics stays on the kernels: ops.bn_momentum / ops.bn_batch_stats)
        # first hidden width: the bottleneck kernels (csrc/btlnk_wide.hip above 16) and the first block's input on csrc/mlp_head.hip (HMAX 64)
        return len(hs) >= 1 and hs[0] <= 64 and all(h <= 64 for h in hs[1:]) and self.output_size <= 64

    def blocks(self):
        """[(bn, linear), ...]: the [BatchNorm1d, ReLU, Linear] blocks behind the first Linear."""
        return [(self.net[3 * i + 1], self.net[3 * i + 3]) for i in range(len(self.hidden_layers))]

    def forward_preact(self, U: Tensor, slope, ws, first_fn) -> Tensor:
        """U: pre-activation of the encoder's last layer (PReLU `slope` applied on load; None: already activated);
        `first_fn(U, slope, W, b, ws)` is the bottleneck autograd node (models/sts/ae.py)."""
        y = first_fn(U, slope, self.net[0].weight, self.net[0].bias, ws)
        for bn, lin in self.blocks():
            y = _MLPHeadFn.apply(y, bn.weight, bn.bias, lin.weight, lin.bias, bn, self.training)
        return y

    def forward(self, X: Tensor) -> Tensor:
        return self.net(X)
