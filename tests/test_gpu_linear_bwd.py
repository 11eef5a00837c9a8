"""``vm_linear_wgrad`` / ``vm_linear_dgrad`` raw and through ``kernels.linear_fn`` under autograd
against float64 matmuls of the same bf16 operands (tests/linear_bwd_ref.py):
``|got - ref| <= tol (rms(ref) + |ref|)``, tol 1e-4 for values stored in fp32, 2e-2 for values
stored in bf16 against the reference rounded once to bf16 — the project's backward bounds.

Raw wgrad: m in {1, 65, S + 1, 3 S + 5} (S = 256, the plan's slice rows: one short slice, a
row-block tail, a one-row second slice, four slices with a tail), n in {8, 72, 192, 2304}, k in
{64, 192, 576, 1152}, dw in fp32 and bf16, thinned by cycling with every value of every axis
present (asserted in test_linear_bwd_cpu.py), VideoMamba-M's two projections and one case on
column-sliced views.  Raw dgrad: (n, k) in {(768, 192), (192, 384), (2304, 576), (576, 1152)},
m in {1, 129, 300}; bit-equal to ``kernels.linear`` on the transposed weight wherever n is one
of the forward's reduction lengths, and a row's bits do not depend on m — also at m = 36,000,
where the 36-step dgrad takes the persistent kernel.

Worst |got - ref| / (tol (rms + |ref|)) of the MI355X run over all cases (1.0 = the bound):

    stored    dw (raw)   dx (raw)   linear_fn dx   linear_fn dw
    fp32      0.006      -          -              -
    bf16      0.176      0.186      0.176          0.245
"""

import pytest
import torch
import torch.nn.functional as F

import linear_bwd_ref as lbr
import train_bwd_ref as tbr
from videomamba_amd import kernels as K
from videomamba_amd import options

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
S = lbr.S


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _wide(t, pad):
    """t as a column-sliced view of a wider buffer (row stride t.shape[1] + pad)."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), 7.0, dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]]


def _wid(c):
    m, n, k, dt, strided = c
    return f"m{m}-n{n}-k{k}-{'fp32' if dt == F32 else 'bf16'}{'-strided' if strided else ''}"


@pytest.mark.parametrize("case", lbr.wgrad_cases(), ids=_wid)
def test_raw_wgrad_matches_float64(case):
    m, n, k, dt, strided = case
    dy, x = lbr.wgrad_inputs(m, n, k)
    if strided:
        dyd, xd = _wide(dy, 8), _wide(x, 64)
        dw = _wide(torch.zeros(n, k, dtype=dt), 8)
        assert dyd.stride(0) > n and xd.stride(0) > k and dw.stride(0) > k
    else:
        dyd, xd = dy.to(DEV), x.to(DEV)
        dw = torch.full((n, k), float("nan"), dtype=dt, device=DEV)
    K.linear_wgrad_raw(dyd, xd, dw, m, n, k, _stream())
    tol, ref = lbr.stored_ref(lbr.wgrad_ref64(m, n, k), dt)
    worst = tbr.assert_within_rms(dw, ref, tol, "dw")
    print(f"\nwgrad {_wid(case)}: dw={worst:.3f}")
    if strided:  # the columns past the width are the caller's
        assert bool((dw._base[:, k:] == 7.0).all())
    # a second call, and a call with another, larger workspace: the same bits
    dw2 = torch.empty((n, k), dtype=dt, device=DEV)
    K.linear_wgrad_raw(dyd, xd, dw2, m, n, k, _stream())
    ws = torch.full((K.linear_wgrad_workspace_bytes(m, n, k) + 4096,), 0xA5, dtype=torch.uint8,
                    device=DEV)
    dw3 = torch.empty((n, k), dtype=dt, device=DEV)
    K.linear_wgrad_raw(dyd, xd, dw3, m, n, k, _stream(), workspace=ws)
    assert torch.equal(dw2, dw.contiguous()) and torch.equal(dw3, dw2)


def test_raw_wgrad_of_no_rows_is_zero():
    dw = torch.full((72, 192), float("nan"), dtype=BF16, device=DEV)
    K.linear_wgrad_raw(torch.empty(0, 72, dtype=BF16, device=DEV),
                       torch.empty(0, 192, dtype=BF16, device=DEV), dw, 0, 72, 192, _stream())
    assert bool((dw == 0).all())


@pytest.mark.parametrize("nk", lbr.DG_NK, ids=lambda nk: f"n{nk[0]}-k{nk[1]}")
def test_raw_dgrad_matches_float64_and_the_forward_kernels(nk):
    n, k = nk
    got = {}
    for m in lbr.DG_M:
        dy, w = lbr.dgrad_inputs(m, n, k)
        wT = w.to(DEV).t().contiguous()
        dx = K.linear_dgrad(dy.to(DEV), wT)
        assert dx.shape == (m, k) and dx.dtype == BF16
        tol, ref = lbr.stored_ref(lbr.dgrad_ref64(m, n, k), BF16)
        worst = tbr.assert_within_rms(dx, ref, tol, "dx")
        print(f"\ndgrad m{m}-n{n}-k{k}: dx={worst:.3f}")
        if n in lbr.FWD_K:
            assert torch.equal(dx, K.linear(dy.to(DEV), wT))
        got[m] = dx
    # a row's bits do not depend on m: the same dy rows in a longer call
    dy300, w = lbr.dgrad_inputs(300, n, k)
    wT = w.to(DEV).t().contiguous()
    short = K.linear_dgrad(dy300[:129].to(DEV), wT)
    assert torch.equal(got[300][:129], short)
    one = K.linear_dgrad(dy300[:1].to(DEV), wT)
    assert torch.equal(got[300][:1], one)


def test_raw_dgrad_persistent_form_has_the_row_bits_of_the_short_call():
    """m = 36,000 rows of VideoMamba-M's in_proj dgrad (n = 2304: the 36 K steps only the dgrad
    runs; 141 row blocks x 3 tiles, past 1.5 tiles per CU of a 256-CU chip, with a row-block
    tail) take the persistent kernel; 129- and 300-row calls take the LDS-DMA tiles, which the
    float64 cases above check.  A row's bits do not depend on m, so the long call's first and
    last rows equal the short calls on the same dy rows."""
    m, n, k = 36000, 2304, 576
    _, w = lbr.dgrad_inputs(300, n, k)
    wT = w.to(DEV).t().contiguous()
    g = torch.Generator(device=DEV).manual_seed(11)
    dy = torch.randn(m, n, generator=g, device=DEV).to(BF16)
    dx = K.linear_dgrad(dy, wT)
    assert torch.equal(dx[:129], K.linear_dgrad(dy[:129], wT))
    assert torch.equal(dx[m - 300:], K.linear_dgrad(dy[m - 300:], wT))
    tol, ref = lbr.stored_ref(dy[17000:17040].cpu().to(F64) @ w.to(F64), BF16)
    tbr.assert_within_rms(dx[17000:17040], ref, tol, "dx rows 17000-17039")


PAIRS = {"Ti": ((384 * 2, 192), (192, 384)), "M": ((2304, 576), (576, 1152))}  # (n, k)


def _fn_inputs(n, k, seed=5):
    g = torch.Generator().manual_seed(seed + n + k)
    x = torch.randn(2, 37, k, generator=g).to(BF16)
    w = (torch.randn(n, k, generator=g) * k ** -0.5).to(BF16)
    gy = torch.randn(2, 37, n, generator=g).to(BF16)
    return x, w, gy


@pytest.mark.parametrize("nk", [p for pair in PAIRS.values() for p in pair],
                         ids=lambda nk: f"n{nk[0]}-k{nk[1]}")
def test_linear_fn_forward_bits_gradients_and_determinism(nk):
    n, k = nk
    x, w, gy = _fn_inputs(n, k)
    xd = x.to(DEV).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    with options.override(train_gemm="hip"):
        y = K.linear_fn(xd, wd)
    assert _is_hip(y)
    assert y.shape == (2, 37, n) and y.dtype == BF16 and y.requires_grad
    with torch.no_grad():
        plain = K.linear(xd.reshape(-1, k), wd).reshape(2, 37, n)
    assert torch.equal(y, plain)  # the inference GEMM, the same bits
    gx, gw = torch.autograd.grad(y, [xd, wd], gy.to(DEV), retain_graph=True)
    gx2, gw2 = torch.autograd.grad(y, [xd, wd], gy.to(DEV))
    assert gx.shape == xd.shape and gx.dtype == xd.dtype
    assert gw.shape == wd.shape and gw.dtype == wd.dtype
    assert torch.equal(gx, gx2) and torch.equal(gw, gw2), "a second backward gave other bits"
    g64, x64, w64 = gy.to(F64).reshape(-1, n), x.to(F64).reshape(-1, k), w.to(F64)
    tol, ref = lbr.stored_ref(g64 @ w64, BF16)
    wx = tbr.assert_within_rms(gx.reshape(-1, k), ref, tol, "dx")
    tol, ref = lbr.stored_ref(g64.t() @ x64, BF16)
    ww = tbr.assert_within_rms(gw, ref, tol, "dw")
    print(f"\nlinear_fn n{n}-k{k}: dx={wx:.3f} dw={ww:.3f}")


def _is_hip(y):
    """Whether ``y`` came out of the HIP ``Function`` (through its reshape)."""
    seen, todo = set(), [y.grad_fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        if type(f).__name__ == "_LinearBackward":
            return True
        todo += [g for g, _ in f.next_functions]
    return False


def test_linear_fn_honours_needs_input_grad():
    n, k = 768, 192
    x, w, gy = _fn_inputs(n, k)
    calls = []
    real_d, real_w = K.linear_dgrad, K.linear_wgrad_raw
    K.linear_dgrad = lambda *a, **kw: (calls.append("dgrad"), real_d(*a, **kw))[1]
    K.linear_wgrad_raw = lambda *a, **kw: (calls.append("wgrad"), real_w(*a, **kw))[1]
    try:
        with options.override(train_gemm="hip"):
            # a frozen weight: no dw is produced and no wgrad runs
            xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV)
            y = K.linear_fn(xd, wd)
            assert _is_hip(y)
            (gx,) = torch.autograd.grad(y, [xd], gy.to(DEV))
            assert calls == ["dgrad"] and wd.grad is None
            # a leaf input that does not require grad: no dgrad runs
            calls.clear()
            xd, wd = x.to(DEV), w.to(DEV).requires_grad_(True)
            y = K.linear_fn(xd, wd)
            assert _is_hip(y)
            y.backward(gy.to(DEV))
            assert calls == ["wgrad"] and xd.grad is None and wd.grad is not None
            # neither requires grad: the plain forward, no graph
            assert K.linear_fn(x.to(DEV), w.to(DEV)).grad_fn is None
    finally:
        K.linear_dgrad, K.linear_wgrad_raw = real_d, real_w


def test_linear_fn_path_selection():
    """The HIP ``Function`` on a HIP shape under ``train_gemm = "hip"``; ``F.linear``'s own
    grad_fn for fp32 operands, a bias, k = 100 and ``train_gemm = "library"``."""
    n, k = 768, 192
    x, w, _ = _fn_inputs(n, k)
    xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    with options.override(train_gemm="hip"):
        assert _is_hip(K.linear_fn(xd, wd))
        assert _is_hip(K.linear_fn(xd[0, 0], wd))  # a single row (k,)
        lib = {
            "fp32": K.linear_fn(xd.float(), wd.float()),
            "bias": K.linear_fn(xd, wd, torch.zeros(n, dtype=BF16, device=DEV)),
            "k = 100": K.linear_fn(xd[..., :100], wd[:, :100]),
            "n = 100": K.linear_fn(xd, wd[:100]),
        }
    with options.override(train_gemm="library"):
        lib["library"] = K.linear_fn(xd, wd)
    ref = {"fp32": F.linear(xd.float(), wd.float()),
           "bias": F.linear(xd, wd, torch.zeros(n, dtype=BF16, device=DEV)),
           "k = 100": F.linear(xd[..., :100], wd[:, :100]), "n = 100": F.linear(xd, wd[:100]),
           "library": F.linear(xd, wd)}
    for what, y in lib.items():
        assert not _is_hip(y) and y.grad_fn is not None, what
        assert type(y.grad_fn) is type(ref[what].grad_fn), what
        assert torch.equal(y, ref[what]), what


def test_linear_fn_takes_non_contiguous_operands():
    """x a column-sliced view (rows not 16-byte contiguous in k) and dy arriving transposed:
    both are made row-contiguous by torch ops; gradients come back in the inputs' shapes."""
    n, k = 192, 384
    x, w, gy = _fn_inputs(n, k)
    xw = torch.zeros(2, 37, k + 4, dtype=BF16, device=DEV)
    xw[..., 2:k + 2] = x.to(DEV)
    xd = xw[..., 2:k + 2].detach().requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    assert not xd.is_contiguous()
    with options.override(train_gemm="hip"):
        y = K.linear_fn(xd, wd)
    assert _is_hip(y)
    loss_g = gy.to(DEV).transpose(0, 1).contiguous().transpose(0, 1)  # non-contiguous dy
    gx, gw = torch.autograd.grad(y, [xd, wd], loss_g)
    assert gx.shape == xd.shape and gw.shape == wd.shape
    g64 = gy.to(F64).reshape(-1, n)
    tol, ref = lbr.stored_ref(g64 @ w.to(F64), BF16)
    tbr.assert_within_rms(gx.reshape(-1, k), ref, tol, "dx")
    tol, ref = lbr.stored_ref(g64.t() @ x.to(F64).reshape(-1, k), BF16)
    tbr.assert_within_rms(gw, ref, tol, "dw")


def test_raw_calls_leave_sentinel_margins_untouched():
    """One raw vm_linear_wgrad launch (m = S + 1, n = 72, k = 192: two slices, a tile tail in
    n and in k) and one raw vm_linear_dgrad launch with every output and the workspace between
    4 KiB margins of a byte pattern: ordinary in-bounds launches, after which the margins still
    hold it."""
    m, n, k, M = S + 1, 72, 192, 4096
    dy, x = lbr.wgrad_inputs(m, n, k)
    ws_bytes = K.linear_wgrad_workspace_bytes(m, n, k)
    assert ws_bytes == 2 * 4 * n * k

    def guarded(nbytes):
        buf = torch.full((M + nbytes + M,), 0xA5, dtype=torch.uint8, device=DEV)
        return buf, buf[M:M + nbytes]

    dn, dk = 768, 192  # the dgrad: dx (m, dk) from dy (m, dn)
    bufs = {key: guarded(nb) for key, nb in (("dw32", n * k * 4), ("dw16", n * k * 2),
                                             ("ws", ws_bytes), ("dx", m * dk * 2))}
    dw32 = bufs["dw32"][1].view(F32).view(n, k)
    dw16 = bufs["dw16"][1].view(BF16).view(n, k)
    K.linear_wgrad_raw(dy.to(DEV), x.to(DEV), dw32, m, n, k, _stream(), workspace=bufs["ws"][1])
    K.linear_wgrad_raw(dy.to(DEV), x.to(DEV), dw16, m, n, k, _stream(), workspace=bufs["ws"][1])
    dyg, w = lbr.dgrad_inputs(300, dn, dk)
    dx = bufs["dx"][1].view(BF16).view(m, dk)
    K.linear_dgrad(dyg[:m].to(DEV), w.to(DEV).t().contiguous(), out=dx)
    torch.cuda.synchronize()
    for key, (buf, inner) in bufs.items():
        assert bool((buf[:M] == 0xA5).all()) and bool((buf[M + inner.numel():] == 0xA5).all()), key
    tol, ref = lbr.stored_ref(lbr.wgrad_ref64(m, n, k), F32)
    tbr.assert_within_rms(dw32, ref, tol, "dw fp32")
    assert torch.equal(dw16, dw32.to(BF16))  # the same sums, rounded once
    tol, ref = lbr.stored_ref(lbr.dgrad_ref64(300, dn, dk)[:m], BF16)
    tbr.assert_within_rms(dx, ref, tol, "dx")
