"""All five kernel forms of the mixer middle (conv1d + SiLU -> x_proj -> dt_proj) against the
float64 reference of ``mixer_mid_matrix.py``, one test per (form, geometry, option row).

``vm_conv_proj_plan.h`` picks the form from the shape alone; every case names the form it
means to reach and ``test_mixer_mid_matrix_cpu.py`` checks that name against
``plan_conv_proj`` on the host.  Per case:

* every input and output is a view into a larger buffer.  Output buffers are prefilled with
  one bit pattern, which must survive bit for bit in the guard rows before and after the
  output, in the pad columns of padded rows and in the state buffer outside the slice;
* input buffers hold NaN in the guard rows, the pad columns, the z half of xz and the xz
  rows with step >= seqlen, and no output element may be NaN.  (The in_proj form's input is
  ``hn``; its z output is a plain GEMM of every row, so z rows with step >= seqlen are the
  poison's own and are not looked at.)
* u against ``mid_ref64`` on the steps below seqlen; x_dbl against the float64 projection
  of the kernel's own bf16 u, plain dt against that of its own bf16 x_dbl[:, :R]; the
  activated dt against float64 ``softplus(plain bf16 dt + bias)`` of a second run of the
  same case without the activation (u and x_dbl bit-equal between the two); the in_proj
  form's x is the bf16 x half ``K.linear(hn, w_in)`` writes and its z is compared with the
  float64 GEMM of the same operands; the new conv state is exact;
* rows with step >= seqlen: u, x_dbl and plain dt are exactly 0.  The activated dt there is
  what the kernel defines, ``bf16(softplus(0 + dt_bias[d]))`` (softplus(0) without a bias):
  a function of the channel alone, inside the activated-dt bound of float64 softplus(bias);
* one gapped-xz case per token-major form that takes xz (a gap of two rows between the
  batches' xz rows): the wide form honours ``xz_sb`` and must match the reference, the
  split-K and fused forms must refuse the call and write nothing.

Bounds are those of the conv_proj tests of ``test_gpu_parity.py``: u ``2^-7 |ref| + 1e-5``,
x_dbl / plain dt / z ``2^-7 |want| + 1e-3``, activated dt ``2^-8`` relative.

Largest observed share of each bound per form on an MI355X (printed again by every run with
``-s``; "-": the form has no such output):

    form           cases      u   x_dbl      dt  dt_act       z
    wide              97  0.497   0.396   0.396   0.996       -
    split_k           49  0.497   0.395   0.388       -       -
    fused            161  0.497   0.395   0.396       -       -
    in_proj          144  0.497   0.394   0.330       -   0.467
    channel_major     96  0.496   0.396   0.384       -       -

(Cases include each form's gapped-xz case.  Half a bf16 ulp is up to 2^-8 of the value: a
correctly rounded u uses half of its 2^-7 bound, a correctly rounded activated dt all of its
2^-8.)
"""

import pytest
import torch

import mixer_mid_matrix as mm
from videomamba_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
G = 4                       # guard rows before and after every buffer's view
PAT16 = 0x5A5A              # the prefill of bf16 outputs (a finite 1.5e16), as int16
PAT32 = 0x5A5A5A5A          # ... of fp32 outputs, as int32
NAN = float("nan")

RATIOS = {}   # form -> {output: worst share of its bound}
COUNTS = {}   # form -> cases run


@pytest.fixture(autouse=True, scope="module")
def _gpu_and_report():
    assert torch.cuda.is_available(), "gpu-marked tests need a HIP device"
    yield
    print("\nmixer middle matrix: cases and largest |got - ref| / bound   "
          "form  cases  u  x_dbl  dt  dt_act  z")
    for form in mm.FORMS:
        r = RATIOS.get(form, {})
        cells = " ".join(f"{r[k]:6.3f}" if k in r else "     -"
                         for k in ("u", "x_dbl", "dt", "dt_act", "z"))
        print(f"  {form:<14} {COUNTS.get(form, 0):4d} {cells}")


def _record(form, what, ratio):
    r = RATIOS.setdefault(form, {})
    r[what] = max(r.get(what, 0.0), ratio)


def test_every_form_has_cases():
    for form in mm.FORMS:
        n = sum(c.form == form and not c.gapped for c in mm.CASES)
        assert n == len(mm.ROWS[form]) * len(mm.GEOMETRIES[form]) and n >= 16, form
    assert {c.form for c in mm.CASES if c.gapped} == {"wide", "split_k", "fused"}


# --------------------------------------------------------------------------- buffers
class Out:
    """An output: a raw integer buffer prefilled with the pattern and the typed view the
    kernel writes (``rows`` x ``cols`` at row offset G, column 0)."""

    def __init__(self, rows, cols, pitch, dtype=BF16):
        it, pat = (torch.int16, PAT16) if dtype == BF16 else (torch.int32, PAT32)
        self.raw = torch.full((G + rows + G, pitch), pat, dtype=it, device=DEV)
        self.before = self.raw.clone()
        self.view = self.raw.view(dtype)[G: G + rows, :cols]

    def assert_guards_intact(self, what):
        """Everything outside the view still holds the pattern, bit for bit."""
        want = self.before.clone()
        rows, cols = self.view.shape
        want[G: G + rows, :cols] = self.raw[G: G + rows, :cols]
        assert torch.equal(want, self.raw), f"{what}: bytes outside the output were written"

    def assert_untouched(self, what):
        assert torch.equal(self.before, self.raw), f"{what}: a refused call wrote"


class State:
    """A conv state (B, D, W) as a slice of a larger buffer: rows 1 .. B of a
    (B + 1, D + 3, W) buffer at channel offset 1 (padded layout) or of a (B + 2, D, W)
    buffer.  Input states are NaN outside the slice, output states hold the pattern."""

    def __init__(self, case, dtype, values=None):
        B, D, W = case.batch, case.dim, case.width
        pad = case.row.layout == "padded"
        shape = (B + 1, D + 3, W) if pad else (B + 2, D, W)
        sl = (slice(1, B + 1), slice(1, D + 1)) if pad else (slice(1, B + 1), slice(None))
        if values is not None:
            self.raw = torch.full(shape, NAN, dtype=dtype, device=DEV)
            self.view = self.raw[sl]
            self.view.copy_(values.to(DEV))
        else:
            it, pat = (torch.int16, PAT16) if dtype == BF16 else (torch.int32, PAT32)
            self.raw = torch.full(shape, pat, dtype=it, device=DEV)
            self.view = self.raw.view(dtype)[sl]
        self.sl = sl
        self.before = self.raw.clone()
        s = case.strides()
        self.strides = (s["cs_sb"], s["cs_sd"])
        assert (self.view.stride(0), self.view.stride(1)) == self.strides

    def assert_guards_intact(self, what):
        want = self.before.clone()
        want[self.sl] = self.raw[self.sl]
        assert torch.equal(want, self.raw), f"{what}: bytes outside the state slice were written"

    def assert_untouched(self, what):
        assert torch.equal(self.before, self.raw), f"{what}: a refused call wrote"


def _states(case, inp):
    row = case.row
    cs = State(case, inp.state.dtype, inp.state) if inp.state is not None else None
    cso = State(case, BF16 if row.state_out == "bf16" else F32) if row.state_out != "none" else None
    return cs, cso


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _weights(case, inp, with_dt):
    cw = inp.cw.to(DEV)
    cb = inp.cb.to(DEV) if inp.cb is not None else None
    wx_pad = mm.pad_rows(inp.wx, case.e_pad).to(DEV)
    wdt_pad = mm.pad_cols(inp.wdt, case.r_pad).to(DEV) if with_dt else None
    return cw, cb, wx_pad, wdt_pad


# --------------------------------------------------------------------------- runs
def _run_token_major(case, inp, activated):
    """One vm_conv_proj_fwd call on poisoned, guarded buffers.  Returns u, x_dbl, dt as
    (ntok, cols) views, the new state's view (or None) and the list of guarded outputs."""
    s, row = case.strides(), case.row
    B, L, D, E, R, W, n = case.batch, case.out_len, case.dim, case.e, case.r, case.width, case.ntok
    with_dt = row.dt != "none"
    rows_b = s["xz_sb"] // s["xz_sl"]  # out_len, or out_len + the gap
    xz_buf = torch.full((G + B * rows_b + G, s["xz_sl"]), NAN, dtype=BF16, device=DEV)
    xz3 = xz_buf[G: G + B * rows_b].view(B, rows_b, s["xz_sl"])
    xz3[:, : case.seqlen, :D] = inp.x[:, : case.seqlen].to(DEV)
    cs, cso = _states(case, inp)
    cw, cb, wx_pad, wdt_pad = _weights(case, inp, with_dt)
    u, xd = Out(n, D, s["u_sl"]), Out(n, E, s["xd_sl"])
    dt = Out(n, D, s["dt_sl"]) if with_dt else None
    bias = inp.dt_bias.to(DEV) if (activated and inp.dt_bias is not None) else None
    outs = [("u", u), ("x_dbl", xd)] + ([("dt", dt)] if dt else []) + ([("state", cso)] if cso else [])

    def call():
        K.conv_proj_raw(xz_buf[G:], (s["xz_sb"], s["xz_sl"]), cw, cb,
                        cs.view if cs else None, cs.strides if cs else (0, 0),
                        cso.view if cso else None, cso.strides if cso else (0, 0),
                        wx_pad, E, wdt_pad, R, u.view, (L * s["u_sl"], s["u_sl"]),
                        xd.view, (L * s["xd_sl"], s["xd_sl"]),
                        dt.view if dt else None, (L * s["dt_sl"], s["dt_sl"]) if dt else None,
                        L, B, D, case.seqlen, W, _stream(), dt_bias32=bias, dt_softplus=activated)
        torch.cuda.synchronize()

    if case.planned == "none":
        with pytest.raises(RuntimeError, match="xz_sb"):
            call()
        torch.cuda.synchronize()
        for name, o in outs:
            o.assert_untouched(f"{case.id} {name}")
        return None
    call()
    for name, o in outs:
        o.assert_guards_intact(f"{case.id} {name}")
    return dict(u=u.view, x_dbl=xd.view, dt=dt.view if dt else None,
                state=cso.view if cso else None, x=inp.x)


def _run_in_proj(case, inp):
    """vm_in_proj_conv_proj_fwd; x is the bf16 x half vm_linear_fwd writes for the same hn."""
    s, row = case.strides(), case.row
    B, L, D, E, R, W, n, k = (case.batch, case.out_len, case.dim, case.e, case.r, case.width,
                              case.ntok, case.geo.k)
    with_dt = row.dt != "none"
    hn_buf = torch.full((G + n + G, s["ldh"]), NAN, dtype=BF16, device=DEV)
    hn3 = hn_buf[G: G + n].view(B, L, s["ldh"])
    hn3[:, : case.seqlen, :k] = inp.hn[:, : case.seqlen].to(DEV)
    hn = hn_buf[G: G + n, :k]
    w_in = inp.w_in.to(DEV)
    cs, cso = _states(case, inp)
    cw, cb, wx_pad, wdt_pad = _weights(case, inp, with_dt)
    u, xd, z = Out(n, D, s["u_sl"]), Out(n, E, s["xd_sl"]), Out(n, D, s["ldz"])
    dt = Out(n, D, s["dt_sl"]) if with_dt else None
    assert K.in_proj_conv_proj_fits(k, B, L, D, E, case.e_pad, case.r_pad if with_dt else 0, W,
                                    with_dt)
    K.in_proj_conv_proj_raw(hn, w_in, z.view, cw, cb, cs.view if cs else None,
                            cs.strides if cs else (0, 0), cso.view if cso else None,
                            cso.strides if cso else (0, 0), wx_pad, E, wdt_pad, R, u.view,
                            xd.view, dt.view if dt else None, L, B, D, case.seqlen, W, _stream())
    xz_ref = torch.empty(n, 2 * D, dtype=BF16, device=DEV)
    K.linear(hn, w_in, out=xz_ref)
    torch.cuda.synchronize()
    outs = [("u", u), ("x_dbl", xd), ("z", z)] + ([("dt", dt)] if dt else []) \
        + ([("state", cso)] if cso else [])
    for name, o in outs:
        o.assert_guards_intact(f"{case.id} {name}")
    # z of the live rows against the float64 GEMM of the same bf16 operands
    live = torch.arange(L) < case.seqlen
    z3 = z.view.reshape(B, L, D)[:, live].cpu()
    assert not z3.float().isnan().any(), case.id
    want = mm.proj_ref64(inp.hn[:, : case.seqlen].reshape(-1, k), inp.w_in[D:]).reshape(z3.shape)
    _record(case.form, "z", mm.assert_within(z3, want, mm.TOL_PROJ, f"{case.id} z"))
    return dict(u=u.view, x_dbl=xd.view, dt=dt.view if dt else None,
                state=cso.view if cso else None, x=xz_ref[:, :D].reshape(B, L, D).cpu())


def _run_channel_major(case, inp):
    """vm_conv_proj_cm_fwd: rows are channels, columns the batch * out_len tokens."""
    s, row = case.strides(), case.row
    B, L, D, E, R, W, n = case.batch, case.out_len, case.dim, case.e, case.r, case.width, case.ntok
    xz_buf = torch.full((G + 2 * D + G, s["x_sd"]), NAN, dtype=BF16, device=DEV)
    cols = (torch.arange(B)[:, None] * L + torch.arange(case.seqlen)[None]).reshape(-1).to(DEV)
    xz_buf[G: G + D][:, cols] = inp.x[:, : case.seqlen].permute(2, 0, 1).reshape(D, -1).to(DEV)
    cs, cso = _states(case, inp)
    cw, cb, wx_pad, wdt_pad = _weights(case, inp, True)
    u, xd, dt = Out(D, n, s["u_sd"]), Out(E, n, s["xd_sd"]), Out(D, n, s["dt_sd"])
    K.conv_proj_cm_raw(xz_buf[G:], s["x_sd"], cw, cb, cs.view if cs else None,
                       cs.strides if cs else (0, 0), cso.view if cso else None,
                       cso.strides if cso else (0, 0), wx_pad, E, wdt_pad, R, u.view, s["u_sd"],
                       xd.view, s["xd_sd"], dt.view, s["dt_sd"], L, B, D, case.seqlen, W, _stream())
    torch.cuda.synchronize()
    outs = [("u", u), ("x_dbl", xd), ("dt", dt)] + ([("state", cso)] if cso else [])
    for name, o in outs:
        o.assert_guards_intact(f"{case.id} {name}")
    return dict(u=u.view.T, x_dbl=xd.view.T, dt=dt.view.T, state=cso.view if cso else None, x=inp.x)


# --------------------------------------------------------------------------- checks
def _check(case, inp, got, plain=None):
    """``got``: u / x_dbl / dt as (ntok, cols), the new state, and the x the kernel read.
    A softplus row's ``got["dt"]`` is the activated step and ``plain`` the outputs of its
    plain companion (nine sequences, the first ``case.batch`` of them this case's)."""
    B, L, D, R, form, n = case.batch, case.out_len, case.dim, case.r, case.form, case.ntok
    Ls = case.seqlen
    u = got["u"].cpu().reshape(B, L, D)
    xd = got["x_dbl"].cpu()
    dt = got["dt"].cpu() if got["dt"] is not None else None
    for name, t in (("u", u), ("x_dbl", xd), ("dt", dt), ("state", got["state"])):
        assert t is None or not t.float().isnan().any(), f"{case.id}: NaN in {name}"
    ref_u, ref_state = mm.mid_ref64(got["x"][:, :Ls], inp.cw, inp.cb, inp.state)
    _record(form, "u", mm.assert_within(u[:, :Ls], ref_u, mm.TOL_U, f"{case.id} u"))
    # rows with step >= seqlen: exact zeros
    dead = (torch.arange(L) >= Ls).repeat(B)
    assert not u.reshape(-1, D)[dead].float().abs().any(), f"{case.id}: u past seqlen"
    assert not xd[dead].float().abs().any(), f"{case.id}: x_dbl past seqlen"
    want = mm.proj_ref64(u.reshape(-1, D), inp.wx)
    _record(form, "x_dbl", mm.assert_within(xd, want, mm.TOL_PROJ, f"{case.id} x_dbl"))
    if got["state"] is not None:
        assert torch.equal(got["state"].cpu().double(), ref_state), f"{case.id}: new conv state"
    if dt is not None and not case.row.softplus:
        assert not dt[dead].float().abs().any(), f"{case.id}: dt past seqlen"
        want = mm.proj_ref64(xd[:, :R], inp.wdt)
        _record(form, "dt", mm.assert_within(dt, want, mm.TOL_PROJ, f"{case.id} dt"))
    if case.row.softplus:
        assert torch.equal(plain["u"].cpu()[:n].reshape(B, L, D), u), f"{case.id}: u vs plain run"
        assert torch.equal(plain["x_dbl"].cpu()[:n], xd), f"{case.id}: x_dbl vs plain run"
        assert (dt.float() > 0).all(), case.id
        bias = inp.dt_bias.double() if inp.dt_bias is not None else torch.zeros(D, dtype=torch.float64)
        want = mm.softplus64(plain["dt"].cpu()[:n].double() + bias)
        _record(form, "dt_act", mm.assert_within(dt, want, mm.TOL_DT_ACT, f"{case.id} dt_act"))
        if dead.any():  # past seqlen: bf16(softplus(0 + bias[d])), the channel's alone
            rows = dt[dead]
            assert torch.equal(rows, rows[:1].expand_as(rows)), f"{case.id}: dt_act past seqlen"
            mm.assert_within(rows[0], mm.softplus64(bias), mm.TOL_DT_ACT, f"{case.id} dt_act pad")


@pytest.mark.parametrize("case", mm.CASES, ids=lambda c: c.id)
def test_mixer_middle_matches_ref64(case):
    COUNTS[case.form] = COUNTS.get(case.form, 0) + 1
    if case.row.softplus:
        # the same sequences twice: the plain dt of the wide form (batch 9), then the
        # activated step of the first three (a softplus call takes the wide form at any batch)
        big = mm.make_inputs(case, batch=mm.GEOMETRIES["wide"][0].batch)
        companion = case.plain_companion()
        plain = _run_token_major(companion, big, False)
        _check(companion, big, plain)
        inp = big.first(case.batch)
        _check(case, inp, _run_token_major(case, inp, True), plain)
        return
    inp = mm.make_inputs(case)
    if case.form == "in_proj":
        _check(case, inp, _run_in_proj(case, inp))
    elif case.form == "channel_major":
        _check(case, inp, _run_channel_major(case, inp))
    else:
        got = _run_token_major(case, inp, False)
        if case.planned == "none":  # refused, nothing written: checked in the run
            assert got is None
        else:
            _check(case, inp, got)
