"""Selective-scan backward: a float64 autograd reference, the incoming gradients and the
comparator that ``test_scan_bwd_cpu.py`` (no GPU) and ``test_gpu_scan_bwd.py``
(``vm_selective_scan_bwd`` through ``kernels.selective_scan_fn``) share.  A helper module,
not a conftest: it defines no fixtures and no hooks.

Reference
    :func:`scan_fwd64` restates ``scan_matrix.scan_ref64`` on float64 leaves that require
    grad (same operations in the same order, no ``detach``, no in-place writes);
    :func:`grads64` is ``torch.autograd.grad`` of ``<y, dout> + <h_last, dh_last>`` through
    it.  Inputs are ``scan_matrix.make_inputs(row, dt, ..., seed=1)``; ``dout`` (in the
    case's dtype) and ``dh_last`` (fp32) come from a seeded CPU generator
    (:func:`make_dout`).

Rows
    :data:`ROWS` are the eight ``scan_matrix.ROWS`` whose state is not ``bf16_inplace``
    (an in-place state update has no gradient): D / z / bias / softplus on and off against
    none / hl / h0 / h0_hl.  ``dh_last`` exists exactly when the row has an ``h_last``.

Comparator
    ``|got - ref| <= tol (rms(ref) + |ref|)`` per element, rms over the whole reference
    tensor (:func:`rms_ratio`, :func:`assert_within_rms`).  ddelta and dbias have rms 44-60
    and ~4,300 on these inputs with elements that cancel to nearly zero: under the forward's
    plain ``tol + tol |ref|`` torch's own fp32 CPU autograd already uses 0.67 of 1e-4 on
    ddelta, under the rms form at most 0.034 on every gradient.  Tolerances are the
    forward's ``scan_matrix.TOL_Y``: 1e-4 for gradients stored in fp32, 2e-2 for gradients
    stored in bf16 (against the reference rounded once to bf16).
"""

from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

import scan_matrix as sm

ROWS = tuple(r for r in sm.ROWS if r.state != "bf16_inplace")
NAMES = ("u", "delta", "A", "B", "C", "D", "z", "bias", "h0")
# gradients the kernel stores in the case's dtype; the others are always fp32
IN_DTYPE = ("u", "delta", "B", "C", "z")


def scan_fwd64(u, delta, A, B, C, D=None, z=None, bias=None, softplus=False, h0=None):
    """``scan_matrix.scan_ref64`` on float64 tensors as they are (autograd flows through
    every operand).  Returns ``y`` (b, d, l) and ``h_last`` (b, d, n)."""
    b, d, l = u.shape
    n = A.shape[1]
    if bias is not None:
        delta = delta + bias[None, :, None]
    if softplus:
        delta = torch.where(delta > 20.0, delta, torch.log1p(torch.exp(torch.clamp(delta, max=20.0))))
    h = torch.zeros(b, d, n, dtype=torch.float64) if h0 is None else h0
    ys = []
    du = delta * u
    for t in range(l):
        h = torch.exp(delta[:, :, t, None] * A[None]) * h + du[:, :, t, None] * B[:, None, :, t]
        ys.append((h * C[:, None, :, t]).sum(-1))
    y = torch.stack(ys, dim=2) if l else torch.zeros(b, d, 0, dtype=torch.float64)
    if D is not None:
        y = y + u * D[None, :, None]
    if z is not None:
        y = y * (z / (1.0 + torch.exp(-z)))
    return y, h


def leaves64(inp: sm.Inputs) -> Dict[str, Optional[torch.Tensor]]:
    """The case's operands as float64 leaves that require grad (absent ones stay None)."""
    return {k: None if v is None else v.detach().to(torch.float64).clone().requires_grad_(True)
            for k, v in zip(NAMES, inp)}


def make_dout(row: sm.Row, dt: torch.dtype, shape, seed: int = 2
              ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """``dout`` (b, d, l) in ``dt`` and ``dh_last`` (b, d, n) fp32 — None unless the row
    returns a last state — from a seeded CPU generator."""
    Bz, D, L, N = shape
    g = torch.Generator().manual_seed(seed)
    dout = torch.randn(Bz, D, L, generator=g).to(dt)
    dhl = torch.randn(Bz, D, N, generator=g)
    return dout, (dhl if row.has_hl else None)


def grads64(inp: sm.Inputs, row: sm.Row, dout: torch.Tensor,
            dh_last: Optional[torch.Tensor]) -> Dict[str, torch.Tensor]:
    """float64 gradients of ``<y, dout> + <h_last, dh_last>`` with respect to every operand
    the case has, keyed by :data:`NAMES`."""
    lv = leaves64(inp)
    y, h = scan_fwd64(lv["u"], lv["delta"], lv["A"], lv["B"], lv["C"], lv["D"], lv["z"],
                      lv["bias"], row.softplus, lv["h0"])
    loss = (y * dout.to(torch.float64)).sum()
    if dh_last is not None:
        loss = loss + (h * dh_last.to(torch.float64)).sum()
    names = [k for k in NAMES if lv[k] is not None]
    grads = torch.autograd.grad(loss, [lv[k] for k in names])
    return dict(zip(names, grads))


def rms_ratio(got: torch.Tensor, ref: torch.Tensor, tol: float) -> torch.Tensor:
    """|got - ref| / (tol (rms(ref) + |ref|)) per element, in float64 (NaN where either is)."""
    got = got.detach().cpu().to(torch.float64)
    ref = ref.detach().cpu().to(torch.float64)
    rms = ref.pow(2).mean().sqrt() if ref.numel() else ref.new_zeros(())
    return (got - ref).abs() / (tol * (rms + ref.abs()))


def assert_within_rms(got: torch.Tensor, ref: torch.Tensor, tol: float, what: str) -> float:
    """Assert the comparator on every element; returns the largest tolerance ratio."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    r = rms_ratio(got, ref, tol)
    bad = ~(r <= 1.0)
    worst = float(torch.nan_to_num(r, nan=float("inf")).max()) if r.numel() else 0.0
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} elements outside "
                           f"{tol:g} (rms + |ref|), worst {worst:.3g} x the tolerance")
    return worst


def grad_tol_and_ref(name: str, ref: torch.Tensor, dt: torch.dtype) -> Tuple[float, torch.Tensor]:
    """The tolerance of gradient ``name`` in a case of dtype ``dt`` and the reference it is
    held to: stored in ``dt`` -> TOL_Y[dt] against the reference rounded once to ``dt``;
    stored in fp32 (dA, dD, dbias, dh0) -> 1e-4 against the fp32-rounded reference."""
    if name in IN_DTYPE:
        return sm.TOL_Y[dt], sm.round_like(ref, dt).float()
    return sm.TOL_Y[torch.float32], ref.to(torch.float32)
