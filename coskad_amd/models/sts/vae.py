"""Mirror of the reference's models/sts/vae.py (STSVAE) on the HIP path.

Encoder / decoder run on the gfx950 kernels (STSAE); the two small heads (`fc_mean`, `fc_var`) and the
sampler are torch ops on [B, latent] tensors.  The reference imports `power_spherical` (nicola-decao), which is
neither vendored nor pinned: `PowerSpherical` / `HypersphericalUniform` below restate the published
algorithm (De Cao & Aziz, "The Power Spherical distribution", 2020) -- parity unpinned, checked by moments.
"""
from __future__ import annotations

import math
from typing import List, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ..common.components import MLP
from ..graph_layers.stsgcn import _PReLUFn
from .ae import STSAE

Tensor = torch.Tensor


class HypersphericalUniform:
    """Uniform distribution on S^{dim} (dim = latent_dim - 1)."""

    def __init__(self, dim: int, device="cpu") -> None:
        self.dim, self.device = dim, device

    def entropy(self) -> Tensor:
        d = self.dim + 1
        return torch.tensor(math.log(2) + (d / 2) * math.log(math.pi) - math.lgamma(d / 2), device=self.device)


class _BetaDraw(torch.autograd.Function):
    """torch.distributions.Beta(alpha, beta).rsample() for concentration = stack([alpha, beta], -1): the same draw
    (torch._sample_dirichlet) and torch's _Dirichlet_backward, with torch._dirichlet_grad evaluated in float64
    (ops.dirichlet_grad: its float32 device kernel loses the gradient at the concentrations of a wide latent)."""

    @staticmethod
    def forward(ctx, concentration):
        x = torch._sample_dirichlet(concentration)
        ctx.save_for_backward(x, concentration)
        return x

    @staticmethod
    def backward(ctx, grad_output):
        x, concentration = ctx.saved_tensors
        total = concentration.sum(-1, True).expand_as(concentration)
        grad = ops.dirichlet_grad(x, concentration, total, f64=True)
        return grad * (grad_output - (x * grad_output).sum(-1, True))


class PowerSpherical:
    """p(x; mu, kappa) ∝ (1 + mu^T x)^kappa on S^{d-1}; rsample via t ~ 2 Beta(a,b) - 1 and a Householder
    reflection of e1 onto mu (reparameterised through the Beta sample)."""

    def __init__(self, loc: Tensor, scale: Tensor) -> None:
        self.loc, self.scale = loc, scale
        d = loc.shape[-1]
        self.alpha = (d - 1) / 2 + scale
        self.beta = torch.full_like(scale, (d - 1) / 2)

    def rsample(self) -> Tensor:
        d = self.loc.shape[-1]
        if d > 16 and self.alpha.requires_grad:      # (a latent within 16 keeps torch's own float32 gradient)
            z = _BetaDraw.apply(torch.stack([self.alpha, self.beta], -1)).select(-1, 0)
        else:
            z = torch.distributions.Beta(self.alpha, self.beta).rsample()
        t = (2 * z - 1).unsqueeze(-1)
        v = F.normalize(torch.randn(*self.loc.shape[:-1], d - 1, device=self.loc.device, dtype=self.loc.dtype), dim=-1)
        y = torch.cat([t, torch.sqrt(torch.clamp(1 - t * t, min=0)) * v], -1)
        e1 = torch.zeros_like(self.loc)
        e1[..., 0] = 1
        u = F.normalize(e1 - self.loc, dim=-1)
        return y - 2 * (y * u).sum(-1, keepdim=True) * u

    def log_normalizer(self) -> Tensor:
        return -((self.alpha + self.beta) * math.log(2) + torch.lgamma(self.alpha) - torch.lgamma(self.alpha + self.beta)
                 + self.beta * math.log(math.pi))

    def entropy(self) -> Tensor:
        return -(self.log_normalizer() + self.scale * (math.log(2) + torch.digamma(self.alpha)
                                                       - torch.digamma(self.alpha + self.beta)))


def kl_ps_uniform(q: PowerSpherical, p: HypersphericalUniform) -> Tensor:
    """KL(PowerSpherical || HypersphericalUniform) = -H(q) + H(p)  (the term at spherical_vae.py:92)."""
    return -q.entropy() + p.entropy().to(q.scale.device)


class STSVAE(STSAE):
    """STSAE + mean / concentration heads + reparameterised sample (reference vae.py:13-170).
    forward -> (Z, X_rec, (q_Z, p_Z, Z_var))."""

    def __init__(self, *args, distribution: str = 'ps', **kwargs) -> None:
        self.distribution = distribution.lower()
        super().__init__(*args, **kwargs)

    def build_model(self) -> None:
        super().build_model()
        if self.distribution == 'normal':
            self.register_buffer('mean_vector', torch.zeros((1, self.latent_dim)))
        self.register_buffer('threshold_dist', torch.tensor(0, dtype=torch.float32))

    def _set_projector_type(self) -> None:
        input_size = self.hidden_dimension * self.n_frames * self.n_joints
        if self.projector == 'mlp':
            self.btlnk = MLP(input_size=input_size, output_size=self.latent_dim, hidden_size=[self.latent_dim])
            input_size = self.latent_dim
        else:
            self.btlnk = nn.Identity()
            assert self.projector == 'linear', f'Projector type {self.projector} not supported.'
        self.fc_mean = nn.Linear(in_features=input_size, out_features=self.latent_dim)
        if self.distribution == 'normal':
            var_out_features = self.latent_dim
        elif self.distribution == 'ps':
            var_out_features = 1
        else:
            raise ValueError(f'Distribution {self.distribution} not supported.')
        self.fc_var = nn.Linear(in_features=input_size, out_features=var_out_features)

    def encode(self, X: Tensor, return_shape: bool = False):
        assert len(X.shape) == 4, f'Input tensor must have shape [batch_size, input_dim, n_frames, n_joints]. Got {X.shape}'
        X_shape = (X.shape[0], self.hidden_dimension, self.n_frames, self.n_joints, 1)
        Z_mean, var_raw = self._raw_heads(X)
        return self._finish_heads(Z_mean, var_raw, X_shape, return_shape)

    def _raw_heads(self, X: Tensor):
        """-> (fc_mean's output before the normalisation, fc_var's output before softplus + 1)  (vae.py:79-85)"""
        B = X.shape[0]
        n_var = self.fc_var.out_features
        heads = self._heads_fused(X)
        if heads is not None:
            return heads
        U, slope = self.encoder.forward_preact(X)
        if isinstance(self.btlnk, nn.Identity) and self.latent_dim + n_var <= ops.BTLNK_LMAX:   # > 16 rows: csrc/btlnk_wide.hip
            # `linear` projector (vae.py:147-150): both heads read the flattened encoder output -- ONE pass of the
            # bottleneck kernel over U (PReLU fused into the load) with the two weights stacked
            from .ae import _BottleneckFn
            Wc = torch.cat([self.fc_mean.weight, self.fc_var.weight], 0)
            bc = torch.cat([self.fc_mean.bias, self.fc_var.bias], 0)
            H = _BottleneckFn.apply(U, slope, Wc, bc, self._ws)
            Z_mean, var_raw = H[:, :self.latent_dim], H[:, self.latent_dim:]
        else:
            if isinstance(self.btlnk, MLP) and self.btlnk.hip_ok:      # wide Linear + BN/ReLU/Linear tail on the HIP kernels
                from .ae import _BottleneckFn
                Z = self.btlnk.forward_preact(U, slope, self._ws, _BottleneckFn.apply)
            else:
                Z = self.btlnk((U if slope is None else _PReLUFn.apply(U, slope)).reshape(B, -1))
            Z_mean, var_raw = self.fc_mean(Z), self.fc_var(Z)
        return Z_mean, var_raw

    def _finish_heads(self, Z_mean: Tensor, var_raw: Tensor, X_shape, return_shape: bool):
        if self.distribution == 'ps':
            Z_mean = Z_mean / torch.norm(Z_mean, dim=-1, keepdim=True)
        Z_var = F.softplus(var_raw) + 1          # the `+ 1` prevents collapse (vae.py:85)
        if return_shape:
            return Z_mean, Z_var, X_shape
        return Z_mean, Z_var

    def _heads_fused(self, X: Tensor):
        """Eval-mode fast path (no gradient): the fused encoder kernel, then
          `linear` projector (vae.py:147-150): ONE bottleneck pass over its tile-major output with fc_mean | fc_var stacked;
          `mlp` projector (vae.py:141-146): the projector as in STSE, then both small heads as one strided MFMA GEMM.
        -> (Z_mean pre-normalisation, var_raw) or None."""
        L, n_var = self.latent_dim, self.fc_var.out_features
        if isinstance(self.btlnk, nn.Identity):
            r = self._fused_hidden(X, (self.fc_mean.weight, self.fc_var.weight))
            if r is None:
                return None
            Hh, plan = r
            Hd = ops.btlnk_fwd(Hh, plan.wb, torch.cat([self.fc_mean.bias, self.fc_var.bias]), None, ws=self._ws)
            return Hd[:, :L], Hd[:, L:]
        Z = self._project_fused(X)
        if Z is None:
            return None
        Wc = torch.cat([self.fc_mean.weight, self.fc_var.weight], 0)          # [L + n_var, latent]
        Hd = ops.gemm(Z, Wc.t(), bias=torch.cat([self.fc_mean.bias, self.fc_var.bias]), bias_mode=2)
        return Hd[:, :L], Hd[:, L:]

    def reparameterize(self, Z_mean: Tensor, Z_var: Tensor):
        if self.distribution == 'normal':
            q_Z = torch.distributions.normal.Normal(Z_mean, Z_var)
            p_Z = torch.distributions.normal.Normal(torch.zeros_like(Z_mean), torch.ones_like(Z_var))
        else:
            q_Z = PowerSpherical(loc=Z_mean, scale=torch.squeeze(Z_var, dim=-1))
            p_Z = HypersphericalUniform(self.latent_dim - 1, device=Z_mean.device)
        return q_Z, p_Z

    def sample(self, X: Tensor):
        """-> (Z, input_shape, (q_Z, p_Z, Z_var)): forward up to the sampled latent -- every random draw of a forward, in its order"""
        if (not self.training and not torch.is_grad_enabled() and X.is_cuda and self.distribution == 'ps'
                and 2 <= self.latent_dim <= ops.PS_HEAD_LMAX):
            # scoring forward (spherical_vae.py:76-78): normalise, softplus + 1 and the PowerSpherical sample on csrc/vae_head.hip / _wide
            # (two launches around torch's Beta draw and Gaussian direction: the module path's noise streams) instead of ~40
            # element-wise launches
            assert len(X.shape) == 4, f'Input tensor must have shape [batch_size, input_dim, n_frames, n_joints]. Got {X.shape}'
            input_shape = (X.shape[0], self.hidden_dimension, self.n_frames, self.n_joints, 1)
            m_raw, v_raw = self._raw_heads(X)
            Z, _, _, saved = ops.ps_head_forward(m_raw, v_raw)
            Z_var = saved[3].unsqueeze(-1)
            q_Z, p_Z = self.reparameterize(saved[2], Z_var)
            return Z, input_shape, (q_Z, p_Z, Z_var)
        if self._normal_head_on_hip(X):
            # the Gaussian head's scoring forward: softplus + 1 and the sample in ONE launch of csrc/vae_head_normal.hip on the noise
            # Normal.rsample would draw; the distributions are built from the kernel's sigma for the callers that read them
            assert len(X.shape) == 4, f'Input tensor must have shape [batch_size, input_dim, n_frames, n_joints]. Got {X.shape}'
            input_shape = (X.shape[0], self.hidden_dimension, self.n_frames, self.n_joints, 1)
            m_raw, v_raw = self._raw_heads(X)
            Z, _, _, saved = ops.normal_head_forward(m_raw, v_raw)
            Z_var = saved[3]
            q_Z, p_Z = self.reparameterize(m_raw, Z_var)
            return Z, input_shape, (q_Z, p_Z, Z_var)
        Z_mean, Z_var, input_shape = self.encode(X, return_shape=True)
        q_Z, p_Z = self.reparameterize(Z_mean, Z_var)
        return q_Z.rsample(), input_shape, (q_Z, p_Z, Z_var)

    def _normal_head_on_hip(self, X: Tensor) -> bool:
        return (not self.training and not torch.is_grad_enabled() and X.is_cuda and self.distribution == 'normal'
                and 1 <= self.latent_dim <= ops.NORMAL_HEAD_LMAX)

    def cosine_scores(self, X: Tensor, ref: Tensor):
        """1 - cos(ref, z) of the sampled latent per window (spherical_vae.py:76-78,200) from the Gaussian head's scoring form: one
        launch behind the raw heads, z itself is not written.  The noise is sample()'s draw.  None where that form does not apply
        (another distribution, training mode, gradients enabled, a CPU tensor): the caller keeps its torch expression."""
        if not self._normal_head_on_hip(X):
            return None
        m_raw, v_raw = self._raw_heads(X)
        return ops.normal_head_forward(m_raw, v_raw, ref=ref, need_saved=False)[0]

    def _latent(self, X: Tensor):
        Z, input_shape, _ = self.sample(X)
        return Z, input_shape

    def forward(self, X: Tensor):
        Z, input_shape, dists = self.sample(X)
        return Z, self.decode(Z, input_shape=input_shape), dists
