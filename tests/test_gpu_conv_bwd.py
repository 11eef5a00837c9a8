"""``vm_causal_conv1d_bwd`` through ``kernels.causal_conv1d_fn`` under autograd against float64
autograd (tests/train_bwd_ref.py): ``|got - ref| <= tol (rms(ref) + |ref|)``, tol 1e-4 for
gradients stored in fp32 (dweight, dbias, fp32 dx / dconv_state), 2e-2 for gradients stored in
bf16 against the reference rounded once to bf16 — the scan backward's bounds.

Shapes: batch 3 (batch-order sums); D 64, 136 (ragged against a 64-lane wave) and 67 (no
16-byte channel run: the one-channel form); L 1, 3, 4, 5 (below, at, past the width), 61, 62
(either side of the backward's 61-step tile), 63, 64, 65 (either side of the forward's 64-step
tile), 150 (three tiles); width 2, 3, 4; SiLU and bias on and off; conv_state none / fp32 /
bf16; fp32 and bf16.  The product is thinned by cycling the other axes along L, with every
value of every axis present (asserted below).

Worst |got - ref| / (tol (rms + |ref|)) of the MI355X run over all cases (1.0 = the bound):

    stored    out     dx      dconv_state  dweight  dbias
    fp32      0.002   0.004   0.002        0.005    0.007
    bf16      0.009   0.206   0.002        0.006    0.005

(bf16 dx at 0.2 of 2e-2 is the one rounding at the store; dweight / dbias / dconv_state are
always fp32 and sit at 0.2-0.7 % of 1e-4's allowance.)
"""

import itertools

import pytest
import torch

import train_bwd_ref as tbr
from videomamba_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16

LS = (1, 3, 4, 5, 61, 62, 63, 64, 65, 150)


def _cases():
    out = []
    ds, ws, flags, states = (64, 136), (4, 3, 2), ((1, 1), (0, 0), (1, 0), (0, 1)), (None, F32, BF16)
    for i, (L, dt) in enumerate(itertools.product(LS, (F32, BF16))):
        silu, bias = flags[(i // 2 + i) % 4]
        out.append((dt, ds[(i // 2) % 2], L, ws[(i // 2 + i % 2) % 3], bool(silu), bool(bias),
                    states[(i // 2 + 2 * (i % 2)) % 3]))
    # the one-channel form and a second look at the long sequence with the other options
    out += [(F32, 67, 65, 4, True, True, BF16), (BF16, 67, 150, 3, True, False, F32),
            (BF16, 136, 150, 4, True, True, BF16), (F32, 136, 150, 2, False, True, None)]
    return out


CASES = _cases()


def _id(c):
    dt, D, L, W, silu, bias, st = c
    return (f"{'bf16' if dt == BF16 else 'fp32'}-D{D}-L{L}-w{W}-{'silu' if silu else 'lin'}-"
            f"{'bias' if bias else 'nobias'}-cs{'none' if st is None else str(st)[6:]}")


def test_cases_cover_every_value_of_every_axis():
    assert {c[0] for c in CASES} == {F32, BF16}
    assert {c[1] for c in CASES} >= {64, 136}
    assert {c[2] for c in CASES} == set(LS)
    assert {c[3] for c in CASES} == {2, 3, 4}
    assert {c[4] for c in CASES} == {True, False} == {c[5] for c in CASES}
    assert {c[6] for c in CASES} == {None, F32, BF16}
    for dt in (F32, BF16):  # per dtype as well
        sub = [c for c in CASES if c[0] == dt]
        assert {c[3] for c in sub} == {2, 3, 4} and {c[6] for c in sub} == {None, F32, BF16}
        assert {c[4] for c in sub} == {True, False} == {c[5] for c in sub}


def _tm(t):
    """A token-major (b, d, l) leaf: unit channel stride."""
    return t.to(DEV).transpose(1, 2).contiguous().transpose(1, 2).requires_grad_(True)


def _run(ops, dout, silu, tm=True):
    """Forward + gradients on the GPU through the public function; leaves keep the case's
    dtypes."""
    lv = {k: None if v is None else v.to(DEV).requires_grad_(True) for k, v in ops.items()}
    lv["x"] = _tm(ops["x"]) if tm else ops["x"].to(DEV).contiguous().requires_grad_(True)
    out = K.causal_conv1d_fn(lv["x"], lv["weight"], lv["bias"], "silu" if silu else None,
                             conv_state=lv["conv_state"])
    names = [k for k, v in lv.items() if v is not None]
    grads = torch.autograd.grad(out, [lv[k] for k in names], dout.to(DEV), retain_graph=True)
    again = torch.autograd.grad(out, [lv[k] for k in names], dout.to(DEV))
    return out, lv, dict(zip(names, grads)), dict(zip(names, again))


def _reference(ops, dout, silu):
    lv = tbr.leaves64(ops)
    out = tbr.conv_fwd64(lv["x"], lv["weight"], lv["bias"], lv["conv_state"], silu)
    return out, tbr.grads64([out], [dout], lv)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_conv_backward_matches_float64_autograd(case):
    dt, D, L, W, silu, bias, st = case
    ops, dout = tbr.conv_inputs(3, D, L, W, dt, bias, st)
    ref_out, ref = _reference(ops, dout, silu)
    out, lv, got, again = _run(ops, dout, silu)
    assert out.requires_grad and out.dtype == dt
    # the forward under autograd has the bits of the no_grad call
    with torch.no_grad():
        plain = K.causal_conv1d_fn(lv["x"], lv["weight"], lv["bias"], "silu" if silu else None,
                                   conv_state=lv["conv_state"])
    assert torch.equal(out, plain)
    tol, r = tbr.tol_and_ref(ref_out.detach(), dt)
    worst = {"out": tbr.assert_within_rms(out, r, tol, "out")}
    assert set(got) == set(ref)
    for k, g in got.items():
        assert g.shape == lv[k].shape and g.dtype == lv[k].dtype, k
        assert torch.equal(g, again[k]), f"d{k}: a second backward gave other bits"
        tol, r = tbr.tol_and_ref(ref[k], g.dtype)
        worst["d" + k] = tbr.assert_within_rms(g, r, tol, "d" + k)
    if st is not None:
        assert float(got["conv_state"][..., 0].abs().max()) == 0.0
    print(f"\nconv bwd {_id(case)}: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
def test_channel_major_input_goes_through_the_conversion_path(dt):
    ops, dout = tbr.conv_inputs(3, 136, 65, 4, dt, True, F32)
    _, ref = _reference(ops, dout, True)
    out, lv, got, _ = _run(ops, dout, True, tm=False)
    assert lv["x"].stride(2) == 1 and out.shape == lv["x"].shape
    for k, g in got.items():
        assert g.shape == lv[k].shape and g.dtype == lv[k].dtype, k
        tol, r = tbr.tol_and_ref(ref[k], g.dtype)
        tbr.assert_within_rms(g, r, tol, "d" + k)


def test_returned_conv_state_carries_gradient_and_matches_the_no_grad_call():
    ops, _ = tbr.conv_inputs(2, 64, 3, 4, F32, True, F32)
    x, cs = _tm(ops["x"]), ops["conv_state"].to(DEV).requires_grad_(True)
    w, b = ops["weight"].to(DEV), ops["bias"].to(DEV)
    out, new = K.causal_conv1d_fn(x, w, b, "silu", conv_state=cs, return_conv_state=True)
    with torch.no_grad():
        out0, new0 = K.causal_conv1d_fn(x, w, b, "silu", conv_state=cs, return_conv_state=True)
    assert torch.equal(out, out0) and torch.equal(new, new0) and new.requires_grad
    gx, gcs = torch.autograd.grad(new.sum(), [x, cs])
    assert torch.equal(gx, torch.ones_like(gx))  # L = 3 < width: all of x is in the new state
    assert torch.equal(gcs[..., -1], torch.ones_like(gcs[..., -1])) and float(gcs[..., :3].sum()) == 0.0


def test_width_above_four_is_refused_under_autograd_only():
    x = _tm(torch.randn(2, 64, 16))
    w = torch.randn(64, 5, device=DEV)
    with pytest.raises(NotImplementedError, match="width"):
        K.causal_conv1d_fn(x, w, None, "silu")
    with torch.no_grad():
        assert K.causal_conv1d_fn(x, w, None, "silu").shape == x.shape
    assert not K.causal_conv1d_fn(x.detach(), w, None, "silu").requires_grad


def test_outputs_require_grad_when_an_input_does():
    x = torch.randn(2, 24, 64, device=DEV).transpose(1, 2)
    w = torch.randn(64, 4, device=DEV)
    assert not K.causal_conv1d_fn(x, w, None, "silu").requires_grad
    assert K.causal_conv1d_fn(x, w.clone().requires_grad_(True), None, "silu").requires_grad
    assert K.causal_conv1d_fn(x.clone().requires_grad_(True), w, None, None).requires_grad


def test_raw_call_leaves_sentinel_margins_untouched():
    """One raw vm_causal_conv1d_bwd launch (bf16, D 136, L 150, width 4, bf16 state) with
    every output and the workspace between 4 KiB margins of a byte pattern: an ordinary
    in-bounds launch, after which the margins still hold the pattern."""
    Bz, D, L, W, M = 3, 136, 150, 4, 4096
    ops, dout = tbr.conv_inputs(Bz, D, L, W, BF16, True, BF16)
    x = ops["x"].to(DEV).transpose(1, 2).contiguous().transpose(1, 2)
    do = dout.to(DEV).transpose(1, 2).contiguous().transpose(1, 2)
    cs = ops["conv_state"].to(DEV)
    w, b = ops["weight"].to(DEV), ops["bias"].to(DEV)
    ws_bytes = K.conv_bwd_workspace_bytes(Bz, D, L, W)
    assert ws_bytes > 0

    def guarded(nbytes):
        buf = torch.full((M + nbytes + M,), 0xA5, dtype=torch.uint8, device=DEV)
        return buf, buf[M:M + nbytes]

    bufs = {k: guarded(n) for k, n in (("dx", Bz * L * D * 2), ("dcs", Bz * D * W * 4),
                                       ("dw", D * W * 4), ("db", D * 4), ("ws", ws_bytes))}
    dx = bufs["dx"][1].view(BF16).view(Bz, L, D).transpose(1, 2)
    dcs = bufs["dcs"][1].view(F32).view(Bz, D, W)
    dw, db = bufs["dw"][1].view(F32).view(D, W), bufs["db"][1].view(F32)
    s3 = lambda t: (t.stride(0), t.stride(1), t.stride(2))  # noqa: E731
    K.conv_bwd_raw(x, s3(x), w, b, cs, (cs.stride(0), cs.stride(1)), do, s3(do), dx, s3(dx),
                   dcs, (dcs.stride(0), dcs.stride(1)), dw, db, Bz, D, L, W, True,
                   K.dtype_code(BF16), torch.cuda.current_stream().cuda_stream,
                   workspace=bufs["ws"][1])
    torch.cuda.synchronize()
    for k, (buf, inner) in bufs.items():
        assert bool((buf[:M] == 0xA5).all()) and bool((buf[M + inner.numel():] == 0xA5).all()), k
    _, ref = _reference(ops, dout, True)
    tbr.assert_within_rms(dw, ref["weight"].float(), 1e-4, "dweight")
    tbr.assert_within_rms(db, ref["bias"].float(), 1e-4, "dbias")
    tbr.assert_within_rms(dcs, ref["conv_state"].float(), 1e-4, "dconv_state")
    tbr.assert_within_rms(dx, ref["x"].to(BF16).float(), 2e-2, "dx")
