"""Paired selective scan backward on the GPU: raw ``vm_selective_scan_bidir_bwd`` calls
(``kernels.selective_scan_bidir_bwd_raw``) on ``scan_matrix.make_pair_inputs`` operands.

Every gradient against float64 (tests/scan_bidir_bwd_ref.py, checked on the CPU by
test_scan_bidir_bwd_cpu.py) under ``|got - ref| <= tol (rms(ref) + |ref|)`` with the plain
backward's tolerances: 1e-4 for gradients stored in fp32, 2e-2 for gradients stored in bf16
against the reference rounded once to bf16.  split = 2, dim = 136 (three channel groups, the
last with 8 live lanes), L = 150 in frames of 25 and of 1, L = 13 (under two 8-step chunks,
ragged) and L = 16 in frames of 8; everything present, and one case with D, z, bias,
softplus and the states absent.

Then the entry's own contract: both halves bit-equal with two ``vm_selective_scan_bwd``
calls (the backward half's on ``dout`` gathered into flipped order), equal bits from a second
call and from another workspace, 4 KiB sentinel margins around every output and the
workspace, and ``split = 0``.

Largest ratio to the tolerance over all cases, as printed by ``-s`` on an MI355X: fp32 0.170
(dz, L = 150 / F = 25), bf16 0.167 (dC, L = 150 / F = 1); the parameter gradients of either
direction stay under 0.06.
"""

from types import SimpleNamespace

import pytest
import torch

import scan_bidir_bwd_ref as pbr
import scan_bwd_ref as sbr
import scan_matrix as sm
from videomamba_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
SPLIT, DIM, N = 2, 136, 16
ALL_ON = sm.ROWS[1]  # D, z, bias, softplus, h0 and h_last
ALL_OFF = sm.Row(False, False, False, False, "none")
SEQS = [(150, 25), (150, 1), (13, 1), (16, 8)]  # (L, frame_len)

_dtid = lambda dt: "bf16" if dt == BF16 else "fp32"  # noqa: E731
_CASES = {}
RATIOS = {}  # (row id, dtype id) -> {gradient name: worst ratio}


@pytest.fixture(autouse=True, scope="module")
def _gpu_and_report():
    assert torch.cuda.is_available(), "gpu-marked tests need a HIP device"
    yield
    print("\npaired scan backward: largest |got - ref| / (tol (rms(ref) + |ref|))")
    for (rid, dt), worst in sorted(RATIOS.items()):
        print(f"  {rid:<28} {dt:<5} " + " ".join(f"d{n}={v:.3f}" for n, v in worst.items()))


def _tm(t):
    """Same (b, d, l) values stored token-major (unit channel stride)."""
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def _case(row, dt, L, F):
    """CPU operands, incoming gradients, the float64 reference and the device operands of one
    case, made once."""
    key = (row, dt, L, F)
    if key not in _CASES:
        pi = sm.make_pair_inputs(row, dt, SPLIT, DIM, L, N, seed=1)
        dout, dhl, dhl_b = pbr.make_dout(row, dt, SPLIT, DIM, L, N)
        ref = pbr.grads64_paired(pi, row, dout, dhl, dhl_b, F)
        i = pi.both
        tok = lambda t: None if t is None else _tm(t.to(DEV))  # noqa: E731
        par = lambda t: None if t is None else t.to(DEV).contiguous()  # noqa: E731
        d = SimpleNamespace(u=tok(i.u), delta=tok(i.delta), z=tok(i.z), B=tok(i.B), C=tok(i.C),
                            go=tok(dout), A=par(i.A), D=par(i.D), bias=par(i.bias),
                            h0=par(i.h0), dhl=par(dhl), A_b=par(pi.A_b), D_b=par(pi.D_b),
                            bias_b=par(pi.bias_b), h0_b=par(pi.h0_b), dhl_b=par(dhl_b))
        _CASES[key] = SimpleNamespace(row=row, dt=dt, L=L, F=F, ref=ref, d=d)
    return _CASES[key]


def _alloc(c, rows, states, paired, make):
    """Fresh gradient buffers: per-row ones of ``rows`` rows, state ones of ``states`` rows;
    ``make(shape, dtype)`` allocates (token-major buffers are made (b, l, ch) and viewed)."""
    d, dt, L = c.d, c.dt, c.L
    tok = lambda ch: make((rows, L, ch), dt).transpose(1, 2)  # noqa: E731
    g = dict(u=tok(DIM), delta=tok(DIM), B=tok(N), C=tok(N),
             z=tok(DIM) if d.z is not None else None, A=make((DIM, N), F32),
             D=make((DIM,), F32) if d.D is not None else None,
             bias=make((DIM,), F32) if d.bias is not None else None,
             h0=make((states, DIM, N), F32) if d.h0 is not None else None)
    if paired:
        g.update(A_b=make((DIM, N), F32), D_b=None if g["D"] is None else make((DIM,), F32),
                 bias_b=None if g["bias"] is None else make((DIM,), F32),
                 h0_b=None if g["h0"] is None else make((states, DIM, N), F32))
    return g


def _empty(shape, dtype):
    return torch.empty(shape, dtype=dtype, device=DEV)


def _paired(c, g=None, ws=None, split=SPLIT):
    """One vm_selective_scan_bidir_bwd call over 2 ``split`` rows; returns the gradients."""
    d = c.d
    g = _alloc(c, 2 * SPLIT, SPLIT, True, _empty) if g is None else g
    s3, s2 = K._tm_strides, K.strides2
    K.selective_scan_bidir_bwd_raw(
        d.u, s3(d.u), d.delta, s3(d.delta), d.A, d.B, s3(d.B), d.C, s3(d.C), d.D, d.z, s3(d.z),
        d.bias, c.row.softplus, d.h0, s2(d.h0), d.go, s3(d.go), d.dhl, s2(d.dhl),
        g["u"], s3(g["u"]), g["delta"], s3(g["delta"]), g["z"], s3(g["z"]), g["B"], s3(g["B"]),
        g["C"], s3(g["C"]), g["A"], g["D"], g["bias"], g["h0"], s2(g["h0"]),
        2 * split, DIM, c.L, N, K.dtype_code(c.dt), torch.cuda.current_stream().cuda_stream,
        pair=(split, d.A_b, d.D_b, d.bias_b, d.h0_b, d.dhl_b, g["A_b"], g["D_b"], g["bias_b"],
              g["h0_b"], c.F), workspace=ws)
    return g


def _plain(c, half):
    """vm_selective_scan_bwd on one half alone: rows [0, split) with the forward parameters,
    or rows [split, 2 split) with the backward ones and dout gathered into flipped order."""
    d = c.d
    sl = slice(0, SPLIT) if half == 0 else slice(SPLIT, 2 * SPLIT)
    if half == 0:
        A, D, bias, h0, dhl, go = d.A, d.D, d.bias, d.h0, d.dhl, d.go[sl]
    else:
        A, D, bias, h0, dhl = d.A_b, d.D_b, d.bias_b, d.h0_b, d.dhl_b
        go = _tm(d.go[sl][:, :, pbr.out_rows(c.L, c.F).to(DEV)])
    cut = lambda t: None if t is None else t[sl]  # noqa: E731
    u, delta, z, Bm, Cm = cut(d.u), cut(d.delta), cut(d.z), cut(d.B), cut(d.C)
    g = _alloc(c, SPLIT, SPLIT, False, _empty)
    s3, s2 = K._tm_strides, K.strides2
    K.selective_scan_bwd_raw(
        u, s3(u), delta, s3(delta), A, Bm, s3(Bm), Cm, s3(Cm), D, z, s3(z), bias,
        c.row.softplus, h0, s2(h0), go, s3(go), dhl, s2(dhl),
        g["u"], s3(g["u"]), g["delta"], s3(g["delta"]), g["z"], s3(g["z"]), g["B"], s3(g["B"]),
        g["C"], s3(g["C"]), g["A"], g["D"], g["bias"], g["h0"], s2(g["h0"]),
        SPLIT, DIM, c.L, N, K.dtype_code(c.dt), torch.cuda.current_stream().cuda_stream)
    return g


def _check(c, got):
    worst = RATIOS.setdefault((f"{c.row.id} L={c.L} F={c.F}", _dtid(c.dt)), {})
    present = {k for k, v in got.items() if v is not None}
    assert present == set(c.ref), (present, set(c.ref))
    for name in pbr.NAMES:
        if name not in c.ref:
            continue
        tol, r = pbr.grad_tol_and_ref(name, c.ref[name], c.dt)
        what = f"{c.row.id} {_dtid(c.dt)} L={c.L} F={c.F} d{name}"
        ratio = sbr.assert_within_rms(got[name].float(), r, tol, what)
        print(f"{what}: {ratio:.4f} of the tolerance")
        worst[name] = max(worst.get(name, 0.0), ratio)


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
@pytest.mark.parametrize("L,F", SEQS)
def test_paired_backward_matches_float64(L, F, dt):
    """Every gradient of both directions with all operands present."""
    c = _case(ALL_ON, dt, L, F)
    _check(c, _paired(c))


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
def test_paired_backward_without_optional_operands(dt):
    """No D, z, bias, softplus, h0 or dh_last in either direction (the HAS_Z = false kernels,
    null state pointers)."""
    c = _case(ALL_OFF, dt, 150, 25)
    got = _paired(c)
    assert all(got[k] is None for k in ("D", "z", "bias", "h0", "D_b", "bias_b", "h0_b"))
    _check(c, got)


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
@pytest.mark.parametrize("L,F", [(150, 25), (13, 1)])
def test_paired_halves_are_bit_equal_with_plain_calls(L, F, dt):
    """Rows [0, split): the bits of vm_selective_scan_bwd on those rows alone.  Rows
    [split, 2 split): the bits of vm_selective_scan_bwd on those rows with the backward
    direction's parameters and dout gathered into flipped order."""
    c = _case(ALL_ON, dt, L, F)
    got = _paired(c)
    lo, hi = _plain(c, 0), _plain(c, 1)
    for name in pbr.PER_ROW:
        assert torch.equal(got[name][:SPLIT], lo[name]), f"d{name} forward rows"
        assert torch.equal(got[name][SPLIT:], hi[name]), f"d{name} backward rows"
    for name in pbr.DIRECTION:
        assert torch.equal(got[name], lo[name]), f"d{name}"
        assert torch.equal(got[name + "_b"], hi[name]), f"d{name}_b"
    # the two directions are different problems: equal results would mean one ran twice
    assert not torch.equal(got["A"], got["A_b"])


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
def test_paired_backward_is_deterministic(dt):
    """A second call and a call on a workspace of the caller's give equal bits."""
    c = _case(ALL_ON, dt, 150, 25)
    first = _paired(c)
    again = _paired(c)
    nbytes = K.scan_bwd_workspace_bytes(2 * SPLIT, DIM, c.L, N)
    own = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device=DEV)[256:]
    other = _paired(c, ws=own)
    for name, v in first.items():
        assert torch.equal(v, again[name]), f"d{name}: second call differs"
        assert torch.equal(v, other[name]), f"d{name}: another workspace differs"


def test_paired_backward_writes_only_its_outputs():
    """bf16, everything present, L = 37 in frames of 1: every gradient buffer and the
    workspace inside sentinel-filled allocations with 4 KiB margins on both sides; the margins
    come back untouched and the gradients are right."""
    c = _case(ALL_ON, BF16, 37, 1)
    margin, fill = 4096, 0x5A
    owners = []

    def embedded(shape, dtype):
        n = 1
        for s in shape:
            n *= s
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        buf = torch.full((2 * margin + nbytes,), fill, dtype=torch.uint8, device=DEV)
        owners.append((buf, nbytes))
        return buf[margin:margin + nbytes].view(dtype).view(*shape)

    g = _alloc(c, 2 * SPLIT, SPLIT, True, embedded)
    ws = embedded((K.scan_bwd_workspace_bytes(2 * SPLIT, DIM, c.L, N),), torch.uint8)
    got = _paired(c, g=g, ws=ws)
    torch.cuda.synchronize()
    assert len(owners) == len(pbr.NAMES) + 1
    for buf, nbytes in owners:
        assert bool((buf[:margin] == fill).all()) and bool((buf[margin + nbytes:] == fill).all())
    _check(c, got)


def test_paired_backward_of_an_empty_batch_writes_zeros():
    """split = 0 (batch 0): no scan runs, dA / dD / dbias of both directions are zeros — the
    plain entry's empty behaviour — and nothing else is touched."""
    c = _case(ALL_ON, F32, 13, 1)
    g = _alloc(c, 2 * SPLIT, SPLIT, True, lambda s, dt: torch.full(s, 7.0, dtype=dt, device=DEV))
    got = _paired(c, g=g, split=0)
    torch.cuda.synchronize()
    for name in ("A", "D", "bias", "A_b", "D_b", "bias_b"):
        assert bool((got[name] == 0).all()), f"d{name} of an empty batch"
    for name in ("u", "delta", "B", "C", "z", "h0", "h0_b"):
        assert bool((got[name] == 7.0).all()), f"d{name} written by an empty batch"
