"""Selective-scan option matrix: a float64 reference, the inputs and the case table that
``test_scan_matrix_cpu.py`` (no GPU) and ``test_gpu_scan_matrix.py`` (every kernel form of
``vm_selective_scan_fwd`` / ``vm_selective_scan_bidir_fwd``) share.  A helper module, not a
conftest: it defines no fixtures and no hooks.

Reference
    :func:`scan_ref64` is the recurrence of ``oracle.videomamba_oracle.selective_scan`` in
    float64 on the stored input values (bf16 inputs are upcast, never re-rounded);
    :func:`scan_ref64_paired` is two such runs with the backward half's output rows
    permuted as ``vm_selective_scan_bidir_fwd`` documents.

Inputs (:func:`make_inputs`)
    Every channel has its own step scale ``s_d = logspace(-2.5, 0, D)``: the slow channels
    still carry the entry state to the last step, so a lost ``h0`` shows in ``h_last`` (with
    steps of ~0.3 on every channel it has decayed to nothing by L = 150).  Past L = 150 the
    slow end moves down with the length, ``-2.5 - log10(L / 150)``, so that holds at
    L = 600 too while the fast channels keep full-size steps.  With softplus
    ``delta = 0.5 randn`` and ``bias = log(expm1(0.4 s_d))``; without, the raw step is
    already positive, ``delta = (0.05 + 0.3 |randn|) s_d`` and ``bias = 0.1 s_d rand``.  A
    softplus row WITHOUT a bias folds the same per-channel offset into ``delta`` itself
    (otherwise its steps are ~0.7 on every channel and h0 is invisible again).

Option table (:data:`ROWS`)
    A strength-2 covering array over D / z / bias present or absent, softplus on or off and
    five kinds of state handling; :func:`covering_gaps` lists what a table misses.

Comparator
    ``|got - ref| <= tol + tol |ref|`` per element (:func:`mismatch`, the criterion of
    ``torch.testing.assert_close`` with rtol = atol = tol); :func:`tol_ratio` is the part of
    the tolerance an element uses.  Tolerances are those of ``test_gpu_parity.py``.
"""

from __future__ import annotations

import itertools
import math
from typing import NamedTuple, Optional

import torch

TOL_Y = {torch.float32: 1e-4, torch.bfloat16: 2e-2}
TOL_STATE_F32 = 1e-4
TOL_STATE_BF16 = 1e-2

STATES = ("none", "hl", "h0", "h0_hl", "bf16_inplace")


class Row(NamedTuple):
    """One option combination.  ``state``: "none" (no h0, no h_last), "hl" (no h0, fp32
    h_last), "h0" (fp32 h0, no h_last), "h0_hl" (fp32 h0, separate fp32 h_last),
    "bf16_inplace" (a bf16 state updated in place: h_last aliases h0)."""
    D: bool
    z: bool
    bias: bool
    softplus: bool
    state: str

    @property
    def has_h0(self) -> bool:
        return self.state in ("h0", "h0_hl", "bf16_inplace")

    @property
    def has_hl(self) -> bool:
        return self.state in ("hl", "h0_hl", "bf16_inplace")

    @property
    def state_tol(self) -> float:
        return TOL_STATE_BF16 if self.state == "bf16_inplace" else TOL_STATE_F32

    @property
    def id(self) -> str:
        on = [k for k in ("D", "z", "bias", "softplus") if getattr(self, k)]
        return "+".join(on or ["bare"]) + "-" + self.state


# Each state kind carries one option vector and its complement, so every (state, option)
# pair appears; the vectors' (D, z, softplus) parts fall in the four complement classes, so
# all eight (D, z, softplus) triples appear, and every pair of options is equal in one
# vector and unequal in another, so all four of its combinations appear.
ROWS = (
    Row(False, False, False, False, "h0_hl"),
    Row(True, True, True, True, "h0_hl"),
    Row(False, False, True, True, "none"),
    Row(True, True, False, False, "none"),
    Row(False, True, True, False, "hl"),
    Row(True, False, False, True, "hl"),
    Row(False, True, False, True, "h0"),
    Row(True, False, True, False, "h0"),
    Row(True, True, False, True, "bf16_inplace"),
    Row(False, False, True, False, "bf16_inplace"),
)
MAX_ROWS = 12

_FACTORS = {"D": (False, True), "z": (False, True), "bias": (False, True),
            "softplus": (False, True), "state": STATES}


def covering_gaps(rows) -> list:
    """What ``rows`` lacks of the table's contract, as readable strings (empty: all holds):
    at most :data:`MAX_ROWS` rows, every pair of factors in every combination of its values
    (strength 2), and every (z, softplus) combination with D present and with D absent."""
    gaps = []
    if len(rows) > MAX_ROWS:
        gaps.append(f"{len(rows)} rows > {MAX_ROWS}")
    for fa, fb in itertools.combinations(_FACTORS, 2):
        seen = {(getattr(r, fa), getattr(r, fb)) for r in rows}
        for va, vb in itertools.product(_FACTORS[fa], _FACTORS[fb]):
            if (va, vb) not in seen:
                gaps.append(f"{fa}={va} with {fb}={vb}")
    seen = {(r.D, r.z, r.softplus) for r in rows}
    for t in itertools.product((False, True), repeat=3):
        if t not in seen:
            gaps.append("D=%s with z=%s softplus=%s" % t)
    return gaps


# --------------------------------------------------------------------------- reference
def _f64(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else t.detach().cpu().to(torch.float64)


def scan_ref64(u, delta, A, B, C, D=None, z=None, bias=None, softplus=False, h0=None):
    """float64 selective scan.  u, delta, z: (b, d, l); A: (d, n); B, C: (b, n, l); D, bias:
    (d,); h0: (b, d, n).  Returns float64 ``y`` (b, d, l) and ``h_last`` (b, d, n)."""
    u, delta, A, B, C, D, z, bias, h0 = map(_f64, (u, delta, A, B, C, D, z, bias, h0))
    b, d, l = u.shape
    n = A.shape[1]
    if bias is not None:
        delta = delta + bias[None, :, None]
    if softplus:
        delta = torch.where(delta > 20.0, delta, torch.log1p(torch.exp(torch.clamp(delta, max=20.0))))
    h = torch.zeros(b, d, n, dtype=torch.float64) if h0 is None else h0.clone()
    y = torch.empty(b, d, l, dtype=torch.float64)
    du = delta * u
    for t in range(l):
        h = torch.exp(delta[:, :, t, None] * A[None]) * h + du[:, :, t, None] * B[:, None, :, t]
        y[:, :, t] = (h * C[:, None, :, t]).sum(-1)
    if D is not None:
        y = y + u * D[None, :, None]
    if z is not None:
        y = y * (z / (1.0 + torch.exp(-z)))
    return y, h


def pair_out_row(t: int, L: int, F: int) -> int:
    """Output row of the backward half's step t (``scan_entry``, vm_scan.hip): frames of F
    steps in reversed order, steps within a frame in order; plain reversal for F = 1."""
    return L - 1 - t if F == 1 else t + (L - F) - 2 * F * (t // F)


def scan_ref64_paired(u, delta, A, B, C, D, z, bias, softplus, h0, split, A_b, D_b, bias_b,
                      h0_b, frame_len):
    """The paired entry (``vm_selective_scan_bidir_fwd``): rows [0, split) scan with
    (A, D, bias, h0), rows [split, 2 split) — the backward direction's operands, already in
    flipped step order — with (A_b, D_b, bias_b, h0_b), and their step t lands in output
    row :func:`pair_out_row`.  Returns y (2 split, d, l), h_last, h_last_b (float64)."""
    lo = lambda t: None if t is None else t[:split]  # noqa: E731
    hi = lambda t: None if t is None else t[split:]  # noqa: E731
    y_f, h_f = scan_ref64(lo(u), lo(delta), A, lo(B), lo(C), D, lo(z), bias, softplus, h0)
    y_r, h_b = scan_ref64(hi(u), hi(delta), A_b, hi(B), hi(C), D_b, hi(z), bias_b, softplus,
                          h0_b)
    L = u.shape[2]
    y_b = torch.empty_like(y_r)
    for t in range(L):
        y_b[:, :, pair_out_row(t, L, frame_len)] = y_r[:, :, t]
    return torch.cat([y_f, y_b], 0), h_f, h_b


# --------------------------------------------------------------------------- inputs
class Inputs(NamedTuple):
    """CPU operands of one case: u, delta, B, C, z in the case's dtype, A, D, bias fp32, h0
    fp32 (bf16 for the in-place bf16 state); absent operands are None."""
    u: torch.Tensor
    delta: torch.Tensor
    A: torch.Tensor
    B: torch.Tensor
    C: torch.Tensor
    D: Optional[torch.Tensor]
    z: Optional[torch.Tensor]
    bias: Optional[torch.Tensor]
    h0: Optional[torch.Tensor]

    def ref(self, softplus: bool, **drop):
        """scan_ref64 of these operands; ``drop`` replaces operands (e.g. ``h0=None``)."""
        return scan_ref64(*self._replace(**drop)[:8], softplus, self._replace(**drop).h0)


def make_inputs(row: Row, dt: torch.dtype, Bz: int, D: int, L: int, N: int, seed: int) -> Inputs:
    """The recipe of the module docstring; A, u, B, C, z, D, h0 as ``_rand_scan`` of
    test_gpu_parity.py makes them.  Seeded CPU generator; the row only selects which
    operands exist (and where the per-channel offset of a bias-free softplus row goes)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    u = rn(Bz, D, L)
    noise = rn(Bz, D, L)
    A = -torch.exp(torch.log(torch.arange(1, N + 1).float()).repeat(D, 1) + 0.1 * rn(D, N))
    Bm, Cm, Dv, z = rn(Bz, N, L), rn(Bz, N, L), rn(D), rn(Bz, D, L)
    rnd = torch.rand(D, generator=g)
    h0 = rn(Bz, D, N)
    s_d = torch.logspace(-2.5 - math.log10(max(L, 150) / 150.0), 0.0, D)
    if row.softplus:
        bias = torch.log(torch.expm1(0.4 * s_d))
        delta = 0.5 * noise
        if not row.bias:
            delta = delta + bias[None, :, None]
    else:
        bias = 0.1 * s_d * rnd
        delta = (0.05 + 0.3 * noise.abs()) * s_d[None, :, None]
    if row.state == "bf16_inplace":
        h0 = h0.to(torch.bfloat16)
    return Inputs(u.to(dt), delta.to(dt), A, Bm.to(dt), Cm.to(dt), Dv if row.D else None,
                  z.to(dt) if row.z else None, bias if row.bias else None,
                  h0 if row.has_h0 else None)


class PairInputs(NamedTuple):
    """A paired case: ``both`` holds the 2 split batch rows with the forward direction's
    A / D / bias / h0; the *_b members are the backward direction's own."""
    both: Inputs
    split: int
    A_b: torch.Tensor
    D_b: Optional[torch.Tensor]
    bias_b: Optional[torch.Tensor]
    h0_b: Optional[torch.Tensor]

    def ref(self, softplus: bool, frame_len: int):
        i = self.both
        return scan_ref64_paired(i.u, i.delta, i.A, i.B, i.C, i.D, i.z, i.bias, softplus, i.h0,
                                 self.split, self.A_b, self.D_b, self.bias_b, self.h0_b,
                                 frame_len)


def make_pair_inputs(row: Row, dt: torch.dtype, split: int, D: int, L: int, N: int,
                     seed: int) -> PairInputs:
    """Two directions of ``split`` rows each, with parameter sets of their own; a row
    without D / bias / h0 drops it for both directions."""
    f = make_inputs(row, dt, split, D, L, N, seed)
    r = make_inputs(row, dt, split, D, L, N, seed + 1000)
    cat = lambda a, b: None if a is None else torch.cat([a, b], 0)  # noqa: E731
    both = f._replace(u=cat(f.u, r.u), delta=cat(f.delta, r.delta), B=cat(f.B, r.B),
                      C=cat(f.C, r.C), z=cat(f.z, r.z))
    return PairInputs(both, split, r.A, r.D, r.bias, r.h0)


# --------------------------------------------------------------------------- comparator
def tol_ratio(got: torch.Tensor, ref: torch.Tensor, tol: float) -> torch.Tensor:
    """|got - ref| / (tol + tol |ref|) per element, in float64 (NaN where either is)."""
    got, ref = _f64(got), _f64(ref)
    return (got - ref).abs() / (tol + tol * ref.abs())


def mismatch(got: torch.Tensor, ref: torch.Tensor, tol: float) -> torch.Tensor:
    """Elements that fail ``|got - ref| <= tol + tol |ref|`` (a NaN or an infinite
    difference fails)."""
    return ~(tol_ratio(got, ref, tol) <= 1.0)


def round_like(ref: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    """The float64 reference rounded once to the kernel's output dtype."""
    return ref.to(torch.float32) if dt == torch.float32 else ref.to(torch.float32).to(dt)


def assert_within(got: torch.Tensor, ref: torch.Tensor, tol: float, what: str) -> float:
    """Assert the comparator on every element; returns the largest tolerance ratio."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    r = tol_ratio(got, ref, tol)
    bad = ~(r <= 1.0)
    worst = float(torch.nan_to_num(r, nan=float("inf")).max()) if r.numel() else 0.0
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} elements outside "
                           f"{tol:g} abs+rel, worst {worst:.3g} x the tolerance")
    return worst
