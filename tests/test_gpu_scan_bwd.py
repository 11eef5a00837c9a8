"""Selective scan backward on the GPU: ``vm_selective_scan_bwd`` through
``kernels.selective_scan_fn`` with ``requires_grad`` leaves, every gradient against float64
autograd (tests/scan_bwd_ref.py) under ``|got - ref| <= tol (rms(ref) + |ref|)``: tol 1e-4
for gradients stored in fp32 (all of an fp32 case; dA, dD, dbias, dh0 of a bf16 case), 2e-2
for gradients stored in bf16, against the reference rounded once to bf16.

Main matrix: the eight differentiable rows x {fp32, bf16} at (2, 136, 150, 16) on
token-major views — D = 136 is two full waves and one with 8 live lanes, L = 150 is ragged
against the 8-step chunk — plus forward bits equal to the no-grad call and a second backward
with equal bits.  Then short sequences (L = 1 .. 33: below a chunk, at its boundary, one
past), three batch rows over one wave (the batch-order sums), channel-major operands (the
conversion path), one raw call with every output and the workspace between sentinel margins,
and the two refusals.

Largest ratio to the tolerance per gradient over each group of cases, as printed by ``-s``
on an MI355X:

    group       dtype      du  ddelta      dA      dB      dC      dD      dz   dbias     dh0
    batch3      bf16    0.009   0.001   0.043   0.022   0.011   0.003   0.000   0.018   0.036
    batch3      fp32    0.030   0.031   0.042   0.017   0.041   0.003   0.104   0.029   0.060
    chan-major  bf16    0.000   0.002   0.032   0.073   0.046   0.002   0.035   0.043   0.032
    chan-major  fp32    0.034   0.043   0.035   0.023   0.042   0.002   0.066   0.034   0.043
    matrix      bf16    0.106   0.190   0.033   0.102   0.128   0.004   0.089   0.037   0.048
    matrix      fp32    0.069   0.031   0.034   0.044   0.059   0.006   0.079   0.025   0.063
    short       bf16    0.016   0.061   0.066   0.073   0.117   0.003   0.098   0.043   0.049
    short       fp32    0.037   0.043   0.066   0.023   0.042   0.003   0.066   0.034   0.043

(0.000 = every element equal to the rounded reference.)
"""

import pytest
import torch

import scan_bwd_ref as sbr
import scan_matrix as sm
from videomamba_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
SHAPE = (2, 136, 150, 16)
ALL_ON = sm.ROWS[1]  # D, z, bias, softplus, h0 and h_last

_dtid = lambda dt: "bf16" if dt == BF16 else "fp32"  # noqa: E731
_rowid = lambda r: r.id  # noqa: E731

_CASES = {}  # (row, dtype, shape) -> (inputs, dout, dh_last, float64 gradients), made once
RATIOS = {}  # (group, dtype id) -> {gradient name: worst ratio}


@pytest.fixture(autouse=True, scope="module")
def _gpu_and_report():
    assert torch.cuda.is_available(), "gpu-marked tests need a HIP device"
    yield
    print("\nscan backward: largest |got - ref| / (tol (rms(ref) + |ref|))")
    print("  group       dtype " + " ".join(f"{'d' + n:>7}" for n in sbr.NAMES))
    for (group, dt), worst in sorted(RATIOS.items()):
        cells = " ".join(f"{worst[n]:7.3f}" if n in worst else "      -" for n in sbr.NAMES)
        print(f"  {group:<11} {dt:<5} {cells}")


def _case(row, dt, shape):
    key = (row, dt, shape)
    if key not in _CASES:
        inp = sm.make_inputs(row, dt, *shape, seed=1)
        dout, dhl = sbr.make_dout(row, dt, shape)
        _CASES[key] = (inp, dout, dhl, sbr.grads64(inp, row, dout, dhl))
    return _CASES[key]


def _tm(t):
    """Same (b, d, l) values stored token-major (unit channel stride)."""
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def _leaves(inp, tm):
    """Device leaves that require grad; (b, ., l) operands token-major when ``tm``."""
    out = {}
    for name, t in zip(sbr.NAMES, inp):
        if t is None:
            out[name] = None
            continue
        t = t.to(DEV)
        t = _tm(t) if tm and name in sbr.IN_DTYPE else t.contiguous()
        out[name] = t.requires_grad_(True)
    return out


def _forward(lv, row):
    return K.selective_scan_fn(lv["u"], lv["delta"], lv["A"], lv["B"], lv["C"], lv["D"], lv["z"],
                               lv["bias"], row.softplus, return_last_state=row.has_hl,
                               initial_state=lv["h0"])


def _backward(res, lv, row, dout, dhl, retain=False):
    names = [n for n in sbr.NAMES if lv[n] is not None]
    outs, gouts = ([res[0], res[1]], [dout, dhl]) if row.has_hl else ([res], [dout])
    grads = torch.autograd.grad(outs, [lv[n] for n in names], gouts, retain_graph=retain)
    return dict(zip(names, grads))


def _check_grads(got, ref, lv, dt, group, what):
    worst = RATIOS.setdefault((group, _dtid(dt)), {})
    assert set(got) == set(ref)
    for name, g in got.items():
        assert g.shape == lv[name].shape and g.dtype == lv[name].dtype, (what, name)
        tol, r = sbr.grad_tol_and_ref(name, ref[name], dt)
        ratio = sbr.assert_within_rms(g.float(), r, tol, f"{what} d{name}")
        worst[name] = max(worst.get(name, 0.0), ratio)


def _run_case(row, dt, shape, group, tm=True, twice=False):
    inp, dout, dhl, ref = _case(row, dt, shape)
    what = f"{group} {row.id} {_dtid(dt)} {shape}"
    lv = _leaves(inp, tm)
    dout_d = dout.to(DEV)
    dhl_d = None if dhl is None else dhl.to(DEV)
    res = _forward(lv, row)
    out = res[0] if row.has_hl else res
    assert out.requires_grad and out.dtype == dt and out.shape == inp.u.shape
    got = _backward(res, lv, row, dout_d, dhl_d, retain=twice)
    _check_grads(got, ref, lv, dt, group, what)
    if twice:
        with torch.no_grad():
            ng = _forward(lv, row)
        if row.has_hl:
            assert not ng[0].requires_grad
            assert torch.equal(ng[0], res[0]) and torch.equal(ng[1], res[1]), what
        else:
            assert not ng.requires_grad and torch.equal(ng, res), what
        again = _backward(res, lv, row, dout_d, dhl_d)
        for name in got:
            assert torch.equal(got[name], again[name]), f"{what} d{name}: second backward differs"


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
@pytest.mark.parametrize("row", sbr.ROWS, ids=_rowid)
def test_backward_matrix_matches_float64_autograd(row, dt):
    """Every gradient of every row at (2, 136, 150, 16); the forward's bits are those of the
    no-grad call and a second backward repeats the first bit for bit."""
    _run_case(row, dt, SHAPE, "matrix", twice=True)


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
@pytest.mark.parametrize("L", [1, 5, 16, 17, 24, 33])
def test_backward_short_sequences(L, dt):
    """Below one 8-step chunk, at a chunk boundary and one step past it; L = 24 is the
    allocator-block-filling shape of the forward's carry test."""
    _run_case(ALL_ON, dt, (2, 136, L, 16), "short")


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
def test_backward_batch_order_reduction(dt):
    """Exactly one wave per batch row and three rows: dA / dD / dbias are the sums of three
    per-row partials added in batch order."""
    _run_case(ALL_ON, dt, (3, 64, 40, 16), "batch3", twice=True)


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
@pytest.mark.parametrize("row", [ALL_ON, sm.ROWS[4]], ids=_rowid)
def test_backward_channel_major_inputs(row, dt):
    """Step-contiguous (b, d, l) operands: the conversion to token-major views is a
    differentiable torch op outside the Function, so the gradients have the inputs' shapes
    (and strides' owners) and the same values."""
    _run_case(row, dt, (2, 136, 33, 16), "chan-major", tm=False)


def test_raw_backward_writes_only_its_outputs():
    """One selective_scan_bwd_raw call (bf16, everything present, L = 37) with every gradient
    buffer and the workspace inside sentinel-filled allocations, 4 KiB margins on both
    sides: the margins come back untouched and the gradients are right."""
    row, dt, shape = ALL_ON, BF16, (2, 136, 37, 16)
    Bz, D, L, N = shape
    inp, dout, dhl, ref = _case(row, dt, shape)
    margin, fill = 4096, 0x5A
    owners = []

    def embedded(shape_, dtype):
        n = 1
        for s in shape_:
            n *= s
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        buf = torch.full((2 * margin + nbytes,), fill, dtype=torch.uint8, device=DEV)
        owners.append((buf, nbytes))
        return buf[margin:margin + nbytes].view(dtype).view(*shape_)

    tok = lambda ch: embedded((Bz, L, ch), dt).transpose(1, 2)  # noqa: E731  token-major
    du, ddelta, dz, dB, dC = tok(D), tok(D), tok(D), tok(N), tok(N)
    dA, dD, dbias = embedded((D, N), F32), embedded((D,), F32), embedded((D,), F32)
    dh0 = embedded((Bz, D, N), F32)
    ws_bytes = K.scan_bwd_workspace_bytes(Bz, D, L, N)
    ws = embedded((ws_bytes,), torch.uint8)
    dev = lambda t: _tm(t.to(DEV))  # noqa: E731
    u, delta, z, Bm, Cm, go = (dev(inp.u), dev(inp.delta), dev(inp.z), dev(inp.B), dev(inp.C),
                               dev(dout))
    A, Dv, bias, h0, dhl_d = (t.to(DEV).contiguous() for t in (inp.A, inp.D, inp.bias, inp.h0, dhl))
    s3 = lambda t: (t.stride(0), t.stride(1), t.stride(2))  # noqa: E731
    s2 = lambda t: (t.stride(0), t.stride(1))  # noqa: E731
    K.selective_scan_bwd_raw(u, s3(u), delta, s3(delta), A, Bm, s3(Bm), Cm, s3(Cm), Dv, z, s3(z),
                             bias, True, h0, s2(h0), go, s3(go), dhl_d, s2(dhl_d),
                             du, s3(du), ddelta, s3(ddelta), dz, s3(dz), dB, s3(dB), dC, s3(dC),
                             dA, dD, dbias, dh0, s2(dh0), Bz, D, L, N, K.dtype_code(dt),
                             torch.cuda.current_stream().cuda_stream, workspace=ws)
    torch.cuda.synchronize()
    for buf, nbytes in owners:
        assert bool((buf[:margin] == fill).all()) and bool((buf[margin + nbytes:] == fill).all())
    got = dict(u=du, delta=ddelta, A=dA, B=dB, C=dC, D=dD, z=dz, bias=dbias, h0=dh0)
    for name, g in got.items():
        tol, r = sbr.grad_tol_and_ref(name, ref[name], dt)
        sbr.assert_within_rms(g.float(), r, tol, f"raw d{name}")


def test_grad_path_refusals():
    """An in-place last state has no gradient (ValueError); the backward kernel takes 16
    states only (NotImplementedError).  Without a required gradient both calls still run."""
    inp = sm.make_inputs(ALL_ON, F32, 2, 64, 16, 16, seed=1)
    lv = _leaves(inp, True)
    hl = torch.empty(2, 64, 16, device=DEV)
    with pytest.raises(ValueError):
        K.selective_scan_fn(lv["u"], lv["delta"], lv["A"], lv["B"], lv["C"], lv["D"], lv["z"],
                            lv["bias"], True, return_last_state=True, initial_state=lv["h0"],
                            last_state_out=hl)
    with torch.no_grad():
        K.selective_scan_fn(lv["u"], lv["delta"], lv["A"], lv["B"], lv["C"], lv["D"], lv["z"],
                            lv["bias"], True, return_last_state=True, initial_state=lv["h0"],
                            last_state_out=hl)
    inp8 = sm.make_inputs(ALL_ON, F32, 2, 64, 16, 8, seed=1)
    lv8 = _leaves(inp8, True)
    with pytest.raises(NotImplementedError):
        K.selective_scan_fn(lv8["u"], lv8["delta"], lv8["A"], lv8["B"], lv8["C"], lv8["D"],
                            lv8["z"], lv8["bias"], True)
    d8 = {k: None if v is None else v.detach() for k, v in lv8.items()}
    y = K.selective_scan_fn(d8["u"], d8["delta"], d8["A"], d8["B"], d8["C"], d8["D"], d8["z"],
                            d8["bias"], True)
    assert not y.requires_grad
