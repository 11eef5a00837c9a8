"""Paired selective-scan backward (``vm_selective_scan_bidir_bwd``): the float64 reference
and the incoming gradients that ``test_scan_bidir_bwd_cpu.py`` (no GPU) and
``test_gpu_scan_bidir_bwd.py`` share.  A helper module, not a conftest: it defines no fixtures
and no hooks.

Reference (:func:`grads64_paired`)
    ``scan_bwd_ref.grads64`` on each half: rows [0, split) with the forward direction's
    parameters and their ``dout`` rows as they are; rows [split, 2 split) with the backward
    direction's parameters and their ``dout`` gathered into flipped step order through
    ``scan_matrix.pair_out_row`` (step t's gradient is the one of the output row the forward
    stored step t at).  :func:`grads64_paired_autograd` is the same thing obtained another
    way — float64 autograd through a restatement of the paired forward, ``scan_fwd64`` per half
    plus the row scatter — and the CPU test holds the two to 1e-12.

Gradient names
    :data:`NAMES`: ``scan_bwd_ref.NAMES`` (per-row gradients u, delta, B, C, z over all
    2 split rows; A, D, bias, h0 of the forward direction) plus ``A_b``, ``D_b``, ``bias_b``,
    ``h0_b`` of the backward direction.
"""

from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

import scan_bwd_ref as sbr
import scan_matrix as sm

PER_ROW = sbr.IN_DTYPE  # u, delta, B, C, z: one gradient row per batch row
DIRECTION = ("A", "D", "bias", "h0")  # one gradient per direction
NAMES = sbr.NAMES + tuple(k + "_b" for k in DIRECTION)


def out_rows(L: int, F: int) -> torch.Tensor:
    """idx[t] = the output row of the backward half's step t."""
    return torch.tensor([sm.pair_out_row(t, L, F) for t in range(L)], dtype=torch.long)


def halves(pi: sm.PairInputs) -> Tuple[sm.Inputs, sm.Inputs]:
    """The two directions as plain cases: rows [0, split) with the forward parameters, rows
    [split, 2 split) with the backward direction's."""
    i, s = pi.both, pi.split
    lo = lambda t: None if t is None else t[:s]  # noqa: E731
    hi = lambda t: None if t is None else t[s:]  # noqa: E731
    f = i._replace(u=lo(i.u), delta=lo(i.delta), B=lo(i.B), C=lo(i.C), z=lo(i.z))
    r = i._replace(u=hi(i.u), delta=hi(i.delta), B=hi(i.B), C=hi(i.C), z=hi(i.z), A=pi.A_b,
                   D=pi.D_b, bias=pi.bias_b, h0=pi.h0_b)
    return f, r


def make_dout(row: sm.Row, dt: torch.dtype, split: int, D: int, L: int, N: int, seed: int = 2):
    """``dout`` (2 split, D, L) in ``dt`` — the gradient of the paired forward's output, so
    its backward rows are in un-flipped order — and the two fp32 ``dh_last`` (split, D, N),
    None unless the row returns a last state."""
    dout, dhl = sbr.make_dout(row, dt, (2 * split, D, L, N), seed)
    if dhl is None:
        return dout, None, None
    return dout, dhl[:split].contiguous(), dhl[split:].contiguous()


def flipped_dout(dout: torch.Tensor, split: int, F: int) -> torch.Tensor:
    """The backward half's ``dout`` gathered into flipped step order."""
    return dout[split:][:, :, out_rows(dout.shape[2], F)].contiguous()


def _merge(gf: Dict[str, torch.Tensor], gr: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    out = {}
    for k, v in gf.items():
        out[k] = torch.cat([v, gr[k]], 0) if k in PER_ROW else v
    for k in DIRECTION:
        if k in gr:
            out[k + "_b"] = gr[k]
    return out


def grads64_paired(pi: sm.PairInputs, row: sm.Row, dout: torch.Tensor,
                   dhl: Optional[torch.Tensor], dhl_b: Optional[torch.Tensor],
                   F: int) -> Dict[str, torch.Tensor]:
    """Side A: ``scan_bwd_ref.grads64`` per half, keyed by :data:`NAMES`."""
    f, r = halves(pi)
    gf = sbr.grads64(f, row, dout[:pi.split], dhl)
    gr = sbr.grads64(r, row, flipped_dout(dout, pi.split, F), dhl_b)
    return _merge(gf, gr)


def grads64_paired_autograd(pi: sm.PairInputs, row: sm.Row, dout: torch.Tensor,
                            dhl: Optional[torch.Tensor], dhl_b: Optional[torch.Tensor],
                            F: int) -> Dict[str, torch.Tensor]:
    """Side B: float64 autograd of ``<out, dout> + <h_last, dh_last> + <h_last_b, dh_last_b>``
    through the paired forward restated on leaves: ``scan_fwd64`` per half, the backward
    half's step t scattered to output row ``pair_out_row(t)``."""
    f, r = halves(pi)
    lf, lr = sbr.leaves64(f), sbr.leaves64(r)
    run = lambda lv: sbr.scan_fwd64(lv["u"], lv["delta"], lv["A"], lv["B"], lv["C"], lv["D"],  # noqa: E731
                                    lv["z"], lv["bias"], row.softplus, lv["h0"])
    y_f, h_f = run(lf)
    y_r, h_b = run(lr)
    L = y_r.shape[2]
    idx = out_rows(L, F)
    y_b = torch.zeros_like(y_r).index_copy(2, idx, y_r)  # y_b[:, :, idx[t]] = y_r[:, :, t]
    out = torch.cat([y_f, y_b], 0)
    loss = (out * dout.to(torch.float64)).sum()
    if dhl is not None:
        loss = loss + (h_f * dhl.to(torch.float64)).sum() + (h_b * dhl_b.to(torch.float64)).sum()
    nf = [k for k in sbr.NAMES if lf[k] is not None]
    g = torch.autograd.grad(loss, [lf[k] for k in nf] + [lr[k] for k in nf])
    return _merge(dict(zip(nf, g[:len(nf)])), dict(zip(nf, g[len(nf):])))


def grad_tol_and_ref(name: str, ref: torch.Tensor, dt: torch.dtype):
    """``scan_bwd_ref.grad_tol_and_ref`` for a name of :data:`NAMES`."""
    return sbr.grad_tol_and_ref(name[:-2] if name.endswith("_b") else name, ref, dt)
