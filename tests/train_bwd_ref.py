"""Conv1d and add + norm backward: float64 autograd references and seeded inputs that
``test_train_bwd_cpu.py`` (no GPU), ``test_gpu_conv_bwd.py`` and ``test_gpu_norm_bwd.py``
share.  A helper module, not a conftest: it defines no fixtures and no hooks.

Reference
    :func:`conv_fwd64` restates ``oracle.causal_conv1d`` (depthwise causal conv over
    ``[conv_state | x]``, optional bias and SiLU) and :func:`add_norm_fwd64`
    ``oracle.add_norm`` (RMSNorm / LayerNorm of ``x + residual``, ``prenorm`` on and off) on
    float64 tensors as they are, so autograd flows through every operand.  :func:`grads64`
    is ``torch.autograd.grad`` of ``sum_k <out_k, g_k>`` through either.

Comparator
    ``scan_bwd_ref.rms_ratio`` / ``assert_within_rms``: ``|got - ref| <= tol (rms(ref) +
    |ref|)``, tol 1e-4 for gradients stored in fp32 and 2e-2 for gradients stored in bf16
    (against the reference rounded once to bf16) — the scan backward's bounds;
    :func:`tol_and_ref` picks them by the gradient's storage dtype.
"""

from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from scan_bwd_ref import assert_within_rms, rms_ratio  # noqa: F401  (re-exported)

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
TOL = {F32: 1e-4, BF16: 2e-2}


def conv_fwd64(x, weight, bias=None, conv_state=None, silu=True):
    """x (b, d, l), weight (d, w), bias (d), conv_state (b, d, w): out (b, d, l) in float64,
    out[t] = act(bias + sum_i w[i] e[t - w + 1 + i]) over e = [conv_state | x] (zeros without
    a state)."""
    b, d, l = x.shape
    w = weight.shape[1]
    left = conv_state if conv_state is not None else x.new_zeros((b, d, w))
    e = torch.cat([left, x], dim=-1)  # e[j] of the docstring is column w + j
    out = x.new_zeros((b, d, l))
    for i in range(w):
        out = out + weight[None, :, i, None] * e[..., 1 + i:1 + i + l]
    if bias is not None:
        out = out + bias[None, :, None]
    if silu:
        out = out / (1.0 + torch.exp(-out))
    return out


def add_norm_fwd64(x, residual, weight, bias, eps, is_rms, prenorm):
    """y (and the sum s with ``prenorm``) of the fused add + norm, float64."""
    s = x if residual is None else x + residual
    c = s if is_rms else s - s.mean(-1, keepdim=True)
    y = c * torch.rsqrt(c.pow(2).mean(-1, keepdim=True) + eps) * weight
    if bias is not None:
        y = y + bias
    return (y, s) if prenorm else y


def leaves64(ops: Dict[str, Optional[torch.Tensor]]) -> Dict[str, Optional[torch.Tensor]]:
    return {k: None if v is None else v.detach().cpu().to(F64).clone().requires_grad_(True)
            for k, v in ops.items()}


def grads64(outs: Sequence[torch.Tensor], gs: Sequence[Optional[torch.Tensor]],
            lv: Dict[str, Optional[torch.Tensor]]) -> Dict[str, torch.Tensor]:
    """float64 gradients of ``sum_k <outs[k], gs[k]>`` (a None g contributes nothing) with
    respect to every leaf that is present."""
    loss = sum((o * g.detach().cpu().to(F64)).sum() for o, g in zip(outs, gs) if g is not None)
    names = [k for k, v in lv.items() if v is not None]
    return dict(zip(names, torch.autograd.grad(loss, [lv[k] for k in names])))


def tol_and_ref(ref: torch.Tensor, stored: torch.dtype) -> Tuple[float, torch.Tensor]:
    """The tolerance of a gradient stored in ``stored`` and the reference it is held to (the
    float64 reference rounded once to that dtype)."""
    return TOL[stored], ref.to(stored).to(F32)


def conv_inputs(batch, dim, seqlen, width, dt, bias, state, seed=1):
    """Seeded CPU operands of a conv case: x, dout (b, d, l) in ``dt``; weight (d, w) and
    bias (d) fp32; conv_state (b, d, w) in ``state`` (a dtype) or None."""
    g = torch.Generator().manual_seed(seed)
    ops = {"x": torch.randn(batch, dim, seqlen, generator=g).to(dt),
           "weight": 0.5 * torch.randn(dim, width, generator=g),
           "bias": 0.5 * torch.randn(dim, generator=g) if bias else None,
           "conv_state": (torch.randn(batch, dim, width, generator=g).to(state)
                          if state is not None else None)}
    dout = torch.randn(batch, dim, seqlen, generator=g).to(dt)
    return ops, dout


def norm_inputs(rows, cols, dt, bias, res, seed=1):
    """Seeded CPU operands of an add + norm case: x (rows, cols) in ``dt``, residual in
    ``res`` (a dtype) or None, weight / bias (cols) fp32, and the gradients arriving at y
    (``dt``) and at the sum (fp32; cast by the caller)."""
    g = torch.Generator().manual_seed(seed)
    ops = {"x": torch.randn(rows, cols, generator=g).to(dt),
           "residual": (2.0 * torch.randn(rows, cols, generator=g)).to(res) if res is not None
           else None,
           "weight": 1.0 + 0.2 * torch.randn(cols, generator=g),
           "bias": 0.2 * torch.randn(cols, generator=g) if bias else None}
    dy = torch.randn(rows, cols, generator=g).to(dt)
    ds = torch.randn(rows, cols, generator=g)
    return ops, dy, ds
