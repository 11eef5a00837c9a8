"""Mixer-middle option matrix (conv1d + SiLU -> x_proj -> dt_proj): a float64 reference, the
inputs, the option tables and the geometries that ``test_mixer_mid_matrix_cpu.py`` (no GPU)
and ``test_gpu_mixer_mid_matrix.py`` (all five kernel forms ``vm_conv_proj_plan.h`` picks
from) share.  A helper module, not a conftest: it defines no fixtures and no hooks.

Reference
    :func:`mid_ref64` is ``u = silu(conv1d([state | x]) + bias)`` in float64 on the stored
    input values.  A state of either dtype is first cast to bf16, the rule of
    ``oracle.videomamba_oracle.causal_conv1d`` (``conv_state.to(x.dtype)``).  It also returns
    the new conv state: the last ``width`` raw inputs of ``[state | x]``, left-padded with
    zeros.  The projections are not chained through it: :func:`proj_ref64` projects the
    kernel's own rounded outputs (x_dbl from its bf16 u, dt from its bf16 x_dbl[:, :R]).

Inputs (:func:`make_inputs`)
    x and the state are ``randn`` rounded to their dtype; an fp32 state is NOT pre-rounded
    to bf16, so it holds values bf16 cannot represent.  Conv weight and bias U(+-1/sqrt W)
    in fp32, W_x U(+-1/sqrt D) and W_dt U(+-R^-1/2) in bf16; the softplus bias is the Mamba
    init plus ``linspace(-12, 8, D)`` (both softplus branches).  The in_proj form adds
    ``hn`` (randn, bf16) and ``w_in`` U(+-1/sqrt k).

Option tables (:data:`ROWS`)
    Per form a strength-2 covering array of at most :data:`MAX_ROWS` rows over width, state
    in, state out, conv bias, dt, seqlen and layout; :func:`covering_gaps` lists what a table
    misses.  The softplus dt levels exist for the wide form only, the channel-major entry
    always projects dt.

Geometries (:data:`GEOMETRIES`) and cases (:data:`CASES`)
    Every table runs at its form's geometries, the smallest shapes at which the tiling can
    go wrong; each case names the form it means to reach, and the CPU file checks the name
    against ``plan_conv_proj`` itself (``tests/host/conv_proj_form_of.cpp``).

Comparator
    ``|got - ref| <= rel |ref| + abs`` per element with the bounds the conv_proj tests of
    ``test_gpu_parity.py`` use: u (2^-7, 1e-5), x_dbl / plain dt / z (2^-7, 1e-3), the
    activated dt (2^-8, 0); the new conv state is exact.  :func:`tol_ratio` is the part of
    the bound an element uses.
"""

from __future__ import annotations

import itertools
import math
import zlib
from typing import NamedTuple, Optional

import torch

BF16 = torch.bfloat16
D_STATE = 16

# (rel, abs) of the comparator per output
TOL_U = (2.0 ** -7, 1e-5)
TOL_PROJ = (2.0 ** -7, 1e-3)       # x_dbl, plain dt, z
TOL_DT_ACT = (2.0 ** -8, 0.0)      # activated dt: one bf16 rounding, relative

FORMS = ("wide", "split_k", "fused", "in_proj", "channel_major")
WIDTHS = (1, 2, 3, 4)
SEQLENS = ("one", "width-1", "len-2", "len")
STATES = ("none", "bf16", "fp32")
DTS = ("none", "plain", "softplus_bias", "softplus")
LAYOUTS = ("contiguous", "padded")
MAX_ROWS = 16


class Row(NamedTuple):
    """One option combination.  ``seqlen`` names a level (see :meth:`seqlen_of`); ``dt``:
    "none" (dt == NULL), "plain", "softplus_bias" (activated, with dt_bias), "softplus"
    (activated, dt_bias == NULL); ``layout`` "padded": rows with pad columns (xz_sl = 2D + 8,
    u_sl = dt_sl = D + 8, xd_sl = E + 2) and the states slices of a (B + 1, D + 3, W) buffer."""
    width: int
    seqlen: str
    dt: str
    state_in: str
    state_out: str
    bias: bool
    layout: str

    def seqlen_of(self, out_len: int) -> int:
        return max(1, {"one": 1, "width-1": self.width - 1, "len-2": out_len - 2,
                       "len": out_len}[self.seqlen])

    @property
    def softplus(self) -> bool:
        return self.dt.startswith("softplus")

    @property
    def id(self) -> str:
        return (f"w{self.width}-{self.seqlen}-dt_{self.dt}-in_{self.state_in}-out_{self.state_out}"
                f"-{'bias' if self.bias else 'nobias'}-{self.layout}")


def _dt_levels(form: str) -> tuple:
    if form == "wide":
        return DTS
    return ("plain",) if form == "channel_major" else ("none", "plain")


def factors(form: str) -> dict:
    """The option factors of a form's table and their levels."""
    return {"width": WIDTHS, "seqlen": SEQLENS, "dt": _dt_levels(form), "state_in": STATES,
            "state_out": STATES, "bias": (False, True), "layout": LAYOUTS}


def _table(form: str, idx) -> tuple:
    f = factors(form)
    return tuple(Row(*(f[k][i] for k, i in zip(Row._fields, r))) for r in idx)


# Level indices (width, seqlen, dt, state in, state out, bias, layout), found by a search for
# 16 rows that cover every pair of levels; every row has its own (width, seqlen) pair.
_IDX_WIDE = (
    (0, 0, 3, 1, 1, 1, 0), (0, 1, 2, 2, 0, 0, 1), (0, 2, 0, 0, 1, 0, 0), (0, 3, 1, 1, 2, 0, 1),
    (1, 0, 0, 2, 0, 0, 1), (1, 1, 1, 0, 0, 1, 0), (1, 2, 3, 1, 2, 0, 1), (1, 3, 2, 0, 1, 1, 1),
    (2, 0, 2, 2, 2, 0, 0), (2, 1, 0, 1, 2, 0, 1), (2, 2, 1, 2, 1, 1, 0), (2, 3, 3, 0, 0, 1, 0),
    (3, 0, 1, 0, 2, 0, 0), (3, 1, 3, 2, 1, 0, 1), (3, 2, 2, 1, 0, 1, 1), (3, 3, 0, 2, 2, 1, 1))
_IDX_SMALL = (
    (0, 0, 0, 1, 1, 1, 0), (0, 1, 1, 2, 1, 0, 1), (0, 2, 1, 2, 2, 0, 0), (0, 3, 1, 0, 0, 0, 1),
    (1, 0, 1, 2, 0, 0, 0), (1, 1, 0, 0, 2, 0, 0), (1, 2, 0, 1, 0, 1, 0), (1, 3, 1, 2, 1, 1, 1),
    (2, 0, 1, 2, 2, 1, 0), (2, 1, 1, 1, 0, 1, 1), (2, 2, 1, 0, 1, 0, 1), (2, 3, 0, 1, 2, 1, 0),
    (3, 0, 0, 0, 0, 0, 1), (3, 1, 0, 1, 1, 0, 0), (3, 2, 1, 0, 2, 1, 1), (3, 3, 0, 2, 2, 0, 0))
_IDX_CM = (
    (0, 0, 0, 2, 0, 1, 1), (0, 1, 0, 1, 2, 0, 0), (0, 2, 0, 0, 0, 0, 1), (0, 3, 0, 0, 1, 0, 1),
    (1, 0, 0, 0, 0, 1, 0), (1, 1, 0, 2, 1, 1, 1), (1, 2, 0, 1, 1, 0, 0), (1, 3, 0, 2, 2, 1, 1),
    (2, 0, 0, 1, 2, 1, 1), (2, 1, 0, 0, 0, 0, 1), (2, 2, 0, 2, 2, 1, 0), (2, 3, 0, 1, 1, 0, 0),
    (3, 0, 0, 1, 1, 0, 0), (3, 1, 0, 1, 0, 0, 1), (3, 2, 0, 0, 2, 1, 0), (3, 3, 0, 2, 0, 0, 0))

ROWS = {"wide": _table("wide", _IDX_WIDE), "split_k": _table("split_k", _IDX_SMALL),
        "fused": _table("fused", _IDX_SMALL), "in_proj": _table("in_proj", _IDX_SMALL),
        "channel_major": _table("channel_major", _IDX_CM)}


def covering_gaps(form: str, rows) -> list:
    """What ``rows`` lacks of the form's table contract, as readable strings (empty: all
    holds): at most :data:`MAX_ROWS` rows, only levels the form has, and every pair of
    factors in every combination of its levels (strength 2)."""
    f = factors(form)
    gaps = []
    if len(rows) > MAX_ROWS:
        gaps.append(f"{len(rows)} rows > {MAX_ROWS}")
    for r in rows:
        for k in f:
            if getattr(r, k) not in f[k]:
                gaps.append(f"{k}={getattr(r, k)} is no level of {form}")
    for fa, fb in itertools.combinations(f, 2):
        seen = {(getattr(r, fa), getattr(r, fb)) for r in rows}
        for va, vb in itertools.product(f[fa], f[fb]):
            if (va, vb) not in seen:
                gaps.append(f"{fa}={va} with {fb}={vb}")
    return gaps


# --------------------------------------------------------------------------- geometries
class Geo(NamedTuple):
    """batch (the wide form: 9, and 3 for its softplus rows, which take the wide form at any
    batch), padded length, d_inner, and in_proj's K (0 elsewhere)."""
    batch: int
    out_len: int
    dim: int
    k: int = 0


GEOMETRIES = {
    # 64-row tiles over many short sequences, a ragged last tile, a 64-channel last chunk
    "wide": tuple(Geo(9, L, D) for L in (8, 40, 72) for D in (192, 320)),
    # eight sequence starts in one 64-token tile; a start mid-tile with a half-width last
    # split; ten splits (past the fused form's nine) with starts mid-tile
    "split_k": (Geo(8, 8, 192), Geo(3, 16, 320), Geo(3, 40, 1280)),
    # its minimum length, one and several sequences per 16-row tile walk, nine waves once
    "fused": (Geo(1, 24, 192), Geo(3, 24, 320), Geo(8, 24, 192), Geo(1, 40, 320), Geo(3, 40, 192),
              Geo(8, 40, 320), Geo(1, 72, 192), Geo(3, 72, 320), Geo(8, 72, 192),
              Geo(3, 40, 1152)),
    "in_proj": tuple(Geo(B, L, 384, 192) for L in (56, 64, 120) for B in (1, 3, 8)),
    "channel_major": (Geo(1, 8, 192), Geo(1, 40, 320), Geo(1, 72, 192), Geo(3, 8, 320),
                      Geo(3, 40, 192), Geo(3, 72, 320)),
}

# the row of the gapped-xz cases: xz rows of the batches 2 token rows apart
GAP_ROWS = 2
GAP_ROW = Row(4, "len-2", "plain", "bf16", "bf16", True, "contiguous")
GAP_GEOS = {"wide": Geo(9, 40, 192), "split_k": Geo(3, 16, 320), "fused": Geo(3, 40, 192)}


class Case(NamedTuple):
    """One (form, geometry, row).  ``form`` is the form the case means to reach; a gapped
    case of a small form means to be refused (:attr:`planned` "none")."""
    form: str
    geo: Geo
    row: Row
    gapped: bool = False

    @property
    def batch(self) -> int:
        return 3 if self.form == "wide" and self.row.softplus else self.geo.batch

    @property
    def out_len(self) -> int:
        return self.geo.out_len

    @property
    def dim(self) -> int:
        return self.geo.dim

    @property
    def seqlen(self) -> int:
        return self.row.seqlen_of(self.geo.out_len)

    @property
    def width(self) -> int:
        return self.row.width

    @property
    def r(self) -> int:  # Mamba's dt_rank = ceil(d_model / 16), d_model = dim / 2
        return (self.geo.dim // 2 + 15) // 16

    @property
    def e(self) -> int:
        return self.r + 2 * D_STATE

    @property
    def e_pad(self) -> int:
        return (self.e + 15) // 16 * 16

    @property
    def r_pad(self) -> int:
        return 32 if self.r <= 32 else 64

    @property
    def ntok(self) -> int:
        return self.batch * self.geo.out_len

    @property
    def planned(self) -> str:
        return "none" if self.gapped and self.form != "wide" else self.form

    @property
    def id(self) -> str:
        g = self.geo
        return (f"{self.form}-B{self.batch}L{g.out_len}D{g.dim}-{self.row.id}"
                + ("-gapped" if self.gapped else ""))

    @property
    def seed(self) -> int:
        return zlib.crc32(self.id.encode()) & 0x7FFFFFFF

    def plain_companion(self) -> "Case":
        """The case of a softplus row with a plain dt: at the wide form's own batch (a plain
        dt at batch 3 would take a small form)."""
        return self._replace(row=self.row._replace(dt="plain"))

    def strides(self) -> dict:
        """Element strides of every buffer the entry takes (token-major: row strides and the
        batch stride of xz; channel-major: row = channel strides over the token columns)."""
        D, E, W, n = self.dim, self.e, self.width, self.ntok
        pad = self.row.layout == "padded"
        if self.form == "channel_major":
            s = dict(x_sd=n + 8, u_sd=n + 8, dt_sd=n + 8, xd_sd=n + 2) if pad else \
                dict(x_sd=n, u_sd=n, dt_sd=n, xd_sd=n)
        else:
            s = dict(xz_sl=2 * D + 8, u_sl=D + 8, dt_sl=D + 8, xd_sl=E + 2) if pad else \
                dict(xz_sl=2 * D, u_sl=D, dt_sl=D, xd_sl=E)
            s["xz_sb"] = (self.out_len + (GAP_ROWS if self.gapped else 0)) * s["xz_sl"]
            if self.form == "in_proj":
                s.update(ldh=self.geo.k + (8 if pad else 0), ldw=self.geo.k,
                         ldz=D + (8 if pad else 0))
        s.update(cs_sb=(D + 3) * W if pad else D * W, cs_sd=W)
        return s

    def plan_line(self) -> str:
        """The case as ``tests/host/conv_proj_form_of.cpp`` reads it: the ConvProjPlanIn
        fields its entry fills, in that program's order."""
        s, row = self.strides(), self.row
        want_dt = row.dt != "none"
        in_proj = self.form == "in_proj"
        f = [int(self.form == "channel_major"), int(in_proj), self.batch, self.out_len,
             self.seqlen, self.dim, self.e, self.e_pad, self.r, self.r_pad if want_dt else 0,
             self.width, int(want_dt), int(row.softplus), s.get("xz_sb", 0), s.get("xz_sl", 0),
             s.get("u_sl", 0), int(row.state_in != "none"), int(row.state_out != "none"),
             int(row.state_in == "bf16"), s["cs_sb"], s["cs_sd"], self.geo.k,
             s.get("ldh", 0), s.get("ldw", 0)]
        return " ".join(str(v) for v in f)


def _cases() -> tuple:
    out = []
    for form in FORMS:
        for geo in GEOMETRIES[form]:
            out += [Case(form, geo, row) for row in ROWS[form]]
    out += [Case(form, geo, GAP_ROW, True) for form, geo in GAP_GEOS.items()]
    return tuple(out)


CASES = _cases()


# --------------------------------------------------------------------------- reference
def _f64(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else t.detach().cpu().to(torch.float64)


def mid_ref64(x, weight, bias=None, state=None):
    """float64 causal depthwise conv + SiLU.  x: (b, l, d) token-major; weight: (d, w),
    w in 1..4; bias: (d,) or None; state: (b, d, w) of any dtype or None, cast to bf16 first.
    Returns u (b, l, d) and the new conv state (b, d, w), both float64."""
    x, weight, bias = _f64(x), _f64(weight), _f64(bias)
    b, l, d = x.shape
    w = weight.shape[1]
    if state is not None:
        state = _f64(state.detach().cpu().to(BF16)).transpose(1, 2)  # (b, w, d)
        full = torch.cat([state, x], 1)
    else:
        full = torch.cat([torch.zeros(b, w, d, dtype=torch.float64), x], 1)
    # output step t reads full[t + 1 .. t + w]: the w - 1 inputs before it and its own
    pre = torch.zeros(b, l, d, dtype=torch.float64)
    for k in range(w):
        pre = pre + weight[:, k] * full[:, 1 + k: 1 + k + l]
    if bias is not None:
        pre = pre + bias
    u = pre / (1.0 + torch.exp(-pre))
    return u, full[:, -w:].transpose(1, 2).contiguous()


def proj_ref64(rows, weight):
    """float64 ``rows @ weight^T`` of the stored values (rows: the kernel's own bf16
    output, weight: (out, in) bf16)."""
    return _f64(rows) @ _f64(weight).T


def softplus64(x):
    x = _f64(x)
    return torch.where(x > 20.0, x, torch.log1p(torch.exp(torch.clamp(x, max=20.0))))


# --------------------------------------------------------------------------- inputs
class Inputs(NamedTuple):
    """CPU operands of one case; absent operands are None.  x: (b, out_len, d) bf16 (all
    out_len rows; only the first seqlen are inputs); state: (b, d, w) bf16 or fp32; cw: (d, w),
    cb: (d,) fp32; wx: (e, d), wdt: (d, r) bf16; dt_bias: (d,) fp32; hn: (b, out_len, k),
    w_in: (2 d, k) bf16 for the in_proj form."""
    x: torch.Tensor
    state: Optional[torch.Tensor]
    cw: torch.Tensor
    cb: Optional[torch.Tensor]
    wx: torch.Tensor
    wdt: torch.Tensor
    dt_bias: Optional[torch.Tensor]
    hn: Optional[torch.Tensor]
    w_in: Optional[torch.Tensor]

    def first(self, b: int) -> "Inputs":
        """The same operands with the first ``b`` sequences only."""
        return self._replace(x=self.x[:b], state=None if self.state is None else self.state[:b],
                             hn=None if self.hn is None else self.hn[:b])


def make_inputs(case: Case, batch: Optional[int] = None) -> Inputs:
    """The recipe of the module docstring from a seeded CPU generator; the row only selects
    which operands exist and the state's dtype.  ``batch`` replaces the case's batch (the
    softplus rows: nine sequences, of which the case itself runs the first three)."""
    g = torch.Generator().manual_seed(case.seed)
    B, L, D, W, R, E = batch or case.batch, case.out_len, case.dim, case.width, case.r, case.e
    uni = lambda bound, *s: (torch.rand(*s, generator=g) * 2.0 - 1.0) * bound  # noqa: E731
    x = torch.randn(B, L, D, generator=g).to(BF16)
    state = torch.randn(B, D, W, generator=g)  # fp32 values bf16 cannot hold
    cw = uni(1.0 / math.sqrt(W), D, W)
    cb = uni(1.0 / math.sqrt(W), D)
    wx = uni(1.0 / math.sqrt(D), E, D).to(BF16)
    wdt = uni(R ** -0.5, D, R).to(BF16)
    # Mamba's dt bias: softplus^-1 of dt ~ logU(1e-3, 1e-1), shifted over both branches
    dt0 = torch.exp(torch.rand(D, generator=g) * (math.log(0.1) - math.log(1e-3))
                    + math.log(1e-3)).clamp(min=1e-4)
    dt_bias = dt0 + torch.log(-torch.expm1(-dt0)) + torch.linspace(-12.0, 8.0, D)
    hn = w_in = None
    if case.form == "in_proj":
        k = case.geo.k
        hn = torch.randn(B, L, k, generator=g).to(BF16)
        w_in = uni(1.0 / math.sqrt(k), 2 * D, k).to(BF16)
    row = case.row
    if row.state_in == "none":
        state = None
    elif row.state_in == "bf16":
        state = state.to(BF16)
    return Inputs(x, state, cw, cb if row.bias else None, wx, wdt,
                  dt_bias if row.dt == "softplus_bias" else None, hn, w_in)


def pad_rows(w: torch.Tensor, rows: int) -> torch.Tensor:
    """``w`` with zero rows appended up to ``rows`` (wx_pad)."""
    out = torch.zeros(rows, w.shape[1], dtype=w.dtype)
    out[: w.shape[0]] = w
    return out


def pad_cols(w: torch.Tensor, cols: int) -> torch.Tensor:
    """``w`` with zero columns appended up to ``cols`` (wdt_pad)."""
    out = torch.zeros(w.shape[0], cols, dtype=w.dtype)
    out[:, : w.shape[1]] = w
    return out


# --------------------------------------------------------------------------- comparator
def tol_ratio(got, ref, tol) -> torch.Tensor:
    """|got - ref| / (rel |ref| + abs) per element in float64, tol = (rel, abs); NaN where
    either is NaN; an element equal to a reference of exactly 0 with abs == 0 uses none."""
    got, ref = _f64(got), _f64(ref)
    err = (got - ref).abs()
    bound = tol[0] * ref.abs() + tol[1]
    return torch.where((err == 0) & (bound == 0), torch.zeros_like(err), err / bound)


def mismatch(got, ref, tol) -> torch.Tensor:
    """Elements outside the bound (a NaN or an infinite difference is outside)."""
    return ~(tol_ratio(got, ref, tol) <= 1.0)


def assert_within(got, ref, tol, what: str) -> float:
    """Assert the comparator on every element; returns the largest tolerance ratio."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    r = tol_ratio(got, ref, tol)
    bad = ~(r <= 1.0)
    worst = float(torch.nan_to_num(r, nan=float("inf")).max()) if r.numel() else 0.0
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} elements outside "
                           f"{tol[0]:g} rel + {tol[1]:g} abs, worst {worst:.3g} x the bound")
    return worst
