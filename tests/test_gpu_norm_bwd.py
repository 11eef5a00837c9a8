"""``vm_add_norm_bwd`` through ``kernels.rms_norm_fn`` / ``layer_norm_fn`` under autograd against
float64 autograd (tests/train_bwd_ref.py): ``|got - ref| <= tol (rms(ref) + |ref|)``, tol 1e-4
for gradients stored in fp32 (dweight, dbias, fp32 dx / dresidual), 2e-2 for gradients stored
in bf16 against the reference rounded once to bf16 — the scan backward's bounds.

Shapes: rows 1, 5, 257 (one short workgroup, two, 65 with a one-row tail); cols 64, 100 (the
backward's non-vector form; the forward vectorises it), 192, 576 (VideoMamba-M); RMSNorm and
LayerNorm; bias on and off (LayerNorm);
residual none / fp32 / bf16; ``prenorm`` off, on, and on with a gradient arriving at
``residual_out``; x in fp32 and bf16; one bf16 case with ``residual_in_fp32=False`` and no
residual, so the saved sum is bf16.  The product is thinned by cycling the other axes along
(rows, cols), with every value of every axis present (asserted below).

With a bf16 sum (a bf16 residual, or the bf16-sum case) the reference differentiates through
the same rounded sum: its statistics come from ``s`` as stored.

Worst |got - ref| / (tol (rms + |ref|)) of the MI355X run over all cases (1.0 = the bound):

    stored    y       s       dx      dresidual  dweight  dbias
    fp32      0.002   0.000   0.002   0.002      0.002    0.002
    bf16      0.098   0.000   0.123   0.002      0.002    0.000

(dweight / dbias are always fp32; a bf16 dx is the one rounding at the store.)
"""

import itertools

import pytest
import torch

import train_bwd_ref as tbr
from videomamba_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
EPS = 1e-5

ROWS, COLS = (1, 5, 257), (64, 100, 192, 576)
KINDS = (("rms", False), ("ln", True), ("ln", False))       # (norm, bias)
PRE = ("y", "prenorm", "prenorm_ds")                         # what carries gradient


def _cases():
    out = []
    res = (None, F32, BF16)
    for j, (rows, cols) in enumerate(itertools.product(ROWS, COLS)):
        for o, dt in enumerate((F32, BF16)):
            out.append((dt, rows, cols, *KINDS[(j + o) % 3], res[(j + j // 3 + o) % 3],
                        PRE[(j + 2 * (j // 3) + 2 * o) % 3], True))
    # the saved sum in bf16 without a residual, and VideoMamba-M's block norm both ways
    out += [(BF16, 257, 576, "rms", False, None, "prenorm_ds", False),
            (BF16, 257, 576, "rms", False, F32, "prenorm_ds", True),
            (F32, 257, 576, "ln", True, BF16, "prenorm_ds", True)]
    return out


CASES = _cases()


def _id(c):
    dt, rows, cols, kind, bias, res, pre, rif = c
    return (f"{'bf16' if dt == BF16 else 'fp32'}-r{rows}-c{cols}-{kind}{'-bias' if bias else ''}-"
            f"res{'none' if res is None else str(res)[6:]}-{pre}{'' if rif else '-sum_bf16'}")


def test_cases_cover_every_value_of_every_axis():
    assert {c[0] for c in CASES} == {F32, BF16}
    assert {c[1] for c in CASES} == set(ROWS) and {c[2] for c in CASES} == set(COLS)
    assert {(c[3], c[4]) for c in CASES} == set(KINDS)
    assert {c[5] for c in CASES} == {None, F32, BF16}
    assert {c[6] for c in CASES} == set(PRE)
    assert any(not c[7] and c[0] == BF16 and c[5] is None for c in CASES)
    for dt in (F32, BF16):
        sub = [c for c in CASES if c[0] == dt]
        assert {c[2] for c in sub} == set(COLS) and {c[5] for c in sub} == {None, F32, BF16}
        assert {c[3] for c in sub} == {"rms", "ln"} and {c[6] for c in sub} == set(PRE)


def _sum_dtype(dt, res, rif, prenorm):
    if res is not None:
        return res
    return F32 if (rif or not prenorm) else dt


def _reference(ops, gy, gs, is_rms, sdt):
    """float64 autograd.  The kernel recomputes the statistics from the stored sum, so with a
    bf16 sum the reference runs on that rounded sum (a straight-through rounding: the
    gradient of s passes to x and the residual unchanged)."""
    lv = tbr.leaves64(ops)
    s = lv["x"] if lv["residual"] is None else lv["x"] + lv["residual"]
    if sdt == BF16:
        s = s + (s.detach().to(BF16).to(F64) - s.detach())
    y, s_out = tbr.add_norm_fwd64(s, None, lv["weight"], lv["bias"], EPS, is_rms, True)
    with torch.no_grad():  # the forward itself normalises the unrounded sum
        fwd = tbr.add_norm_fwd64(lv["x"], lv["residual"], lv["weight"], lv["bias"], EPS, is_rms,
                                 True)
    return fwd, tbr.grads64([y, s_out], [gy, gs], lv)


def _run(ops, gy, gs, is_rms, prenorm, rif):
    lv = {k: None if v is None else v.to(DEV).requires_grad_(True) for k, v in ops.items()}
    fn = K.rms_norm_fn if is_rms else K.layer_norm_fn
    res = fn(lv["x"], lv["weight"], lv["bias"], residual=lv["residual"], prenorm=prenorm,
             residual_in_fp32=rif, eps=EPS)
    outs = list(res) if prenorm else [res]
    gl = [gy.to(DEV)] + ([gs.to(DEV).to(outs[1].dtype)] if len(outs) > 1 and gs is not None else [])
    outs_g = outs[:len(gl)]
    names = [k for k, v in lv.items() if v is not None]
    grads = torch.autograd.grad(outs_g, [lv[k] for k in names], gl, retain_graph=True)
    again = torch.autograd.grad(outs_g, [lv[k] for k in names], gl)
    return outs, lv, dict(zip(names, grads)), dict(zip(names, again))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_add_norm_backward_matches_float64_autograd(case):
    dt, rows, cols, kind, bias, res, pre, rif = case
    is_rms, prenorm = kind == "rms", pre != "y"
    ops, gy, gs = tbr.norm_inputs(rows, cols, dt, bias, res)
    sdt = _sum_dtype(dt, res, rif, prenorm)
    gs = gs.to(sdt) if pre == "prenorm_ds" else None
    ref_outs, ref = _reference(ops, gy, gs, is_rms, sdt)
    outs, lv, got, again = _run(ops, gy, gs, is_rms, prenorm, rif)
    assert outs[0].requires_grad and outs[0].dtype == dt
    if prenorm:
        assert outs[1].requires_grad and outs[1].dtype == sdt
    # the forward under autograd has the bits of the no_grad call
    fn = K.rms_norm_fn if is_rms else K.layer_norm_fn
    with torch.no_grad():
        plain = fn(lv["x"], lv["weight"], lv["bias"], residual=lv["residual"], prenorm=prenorm,
                   residual_in_fp32=rif, eps=EPS)
    for o, p in zip(outs, plain if prenorm else [plain]):
        assert torch.equal(o, p)
    worst = {}
    for name, o, r in zip(("y", "s"), outs, ref_outs):
        tol, rr = tbr.tol_and_ref(r.detach(), o.dtype)
        worst[name] = tbr.assert_within_rms(o, rr, tol, name)
    assert set(got) == set(ref)
    for k, g in got.items():
        assert g.shape == lv[k].shape and g.dtype == lv[k].dtype, k
        assert torch.equal(g, again[k]), f"d{k}: a second backward gave other bits"
        tol, r = tbr.tol_and_ref(ref[k], g.dtype)
        worst["d" + k] = tbr.assert_within_rms(g, r, tol, "d" + k)
    print(f"\nnorm bwd {_id(case)}: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


def test_three_dimensional_input_and_non_contiguous_operands():
    """(B, L, C) operands, x a non-contiguous view: gradients come back in the inputs' shapes."""
    ops, gy, gs = tbr.norm_inputs(2 * 24, 64, F32, False, F32)
    xw = torch.zeros(2, 24, 128, device=DEV)
    xw[..., :64] = ops["x"].view(2, 24, 64).to(DEV)
    x = xw[..., :64].detach().requires_grad_(True)
    r = ops["residual"].view(2, 24, 64).to(DEV).requires_grad_(True)
    w = ops["weight"].to(DEV).requires_grad_(True)
    assert not x.is_contiguous()
    y, s = K.rms_norm_fn(x, w, None, residual=r, prenorm=True, residual_in_fp32=True, eps=EPS)
    assert y.shape == x.shape and s.shape == x.shape
    gx, gr, gw = torch.autograd.grad([y, s], [x, r, w], [gy.view(2, 24, 64).to(DEV),
                                                        gs.view(2, 24, 64).to(DEV)])
    _, ref = _reference(ops, gy, gs, True, F32)
    assert gx.shape == x.shape and gr.shape == r.shape
    tbr.assert_within_rms(gx.reshape(48, 64), ref["x"].float(), 1e-4, "dx")
    tbr.assert_within_rms(gr.reshape(48, 64), ref["residual"].float(), 1e-4, "dresidual")
    tbr.assert_within_rms(gw, ref["weight"].float(), 1e-4, "dweight")


def test_in_place_arguments_are_refused_under_autograd_only():
    x = torch.randn(5, 64, device=DEV)
    w = torch.ones(64, device=DEV, requires_grad=True)
    out, ro = torch.empty_like(x), torch.empty_like(x)
    with pytest.raises(ValueError, match="in place"):
        K._norm(x, w, None, None, True, True, EPS, True, out=out)
    with pytest.raises(ValueError, match="in place"):
        K._norm(x, w, None, None, True, True, EPS, True, residual_out=ro)
    with torch.no_grad():
        y, r2 = K._norm(x, w, None, None, True, True, EPS, True, out=out, residual_out=ro)
    assert y is out and r2 is ro


def test_outputs_require_grad_when_an_input_does():
    x = torch.randn(5, 64, device=DEV)
    w = torch.ones(64, device=DEV)
    assert not K.rms_norm_fn(x, w, None, eps=EPS).requires_grad
    assert K.rms_norm_fn(x, w.clone().requires_grad_(True), None, eps=EPS).requires_grad
    y, s = K.layer_norm_fn(x.clone().requires_grad_(True), w, w, residual=x, prenorm=True, eps=EPS)
    assert y.requires_grad and s.requires_grad


def test_raw_call_leaves_sentinel_margins_untouched():
    """One raw vm_add_norm_bwd launch (257 x 100, LayerNorm with bias, bf16 x, fp32 sum: the
    non-vector form, 65 workgroups) with every output and the workspace between 4 KiB margins
    of a byte pattern: an ordinary in-bounds launch, after which the margins still hold it."""
    rows, cols, M = 257, 100, 4096
    ops, gy, gs = tbr.norm_inputs(rows, cols, BF16, True, F32)
    s = (ops["x"].float() + ops["residual"]).to(DEV)
    w, b = ops["weight"].to(DEV), ops["bias"].to(DEV)
    dy, ds = gy.to(DEV), gs.to(DEV)
    ws_bytes = K.add_norm_bwd_workspace_bytes(rows, cols)
    assert ws_bytes > 0

    def guarded(nbytes):
        buf = torch.full((M + nbytes + M,), 0xA5, dtype=torch.uint8, device=DEV)
        return buf, buf[M:M + nbytes]

    bufs = {k: guarded(n) for k, n in (("dx", rows * cols * 2), ("dr", rows * cols * 4),
                                       ("dw", cols * 4), ("db", cols * 4), ("ws", ws_bytes))}
    dx = bufs["dx"][1].view(BF16).view(rows, cols)
    dr = bufs["dr"][1].view(F32).view(rows, cols)
    dw, db = bufs["dw"][1].view(F32), bufs["db"][1].view(F32)
    K.add_norm_bwd_raw(s, w, b, dy, ds, dx, dr, dw, db, rows, cols, EPS, False,
                       torch.cuda.current_stream().cuda_stream, workspace=bufs["ws"][1])
    torch.cuda.synchronize()
    for k, (buf, inner) in bufs.items():
        assert bool((buf[:M] == 0xA5).all()) and bool((buf[M + inner.numel():] == 0xA5).all()), k
    _, ref = _reference(ops, gy, gs, False, F32)
    tbr.assert_within_rms(dw, ref["weight"].float(), 1e-4, "dweight")
    tbr.assert_within_rms(db, ref["bias"].float(), 1e-4, "dbias")
    tbr.assert_within_rms(dr, ref["residual"].float(), 1e-4, "dresidual")
    tbr.assert_within_rms(dx, ref["x"].to(BF16).float(), 2e-2, "dx")
    assert torch.equal(dx, dr.to(BF16))  # the same values, each rounded once
