"""GPU agreement of the fits queries with the entries they answer for: where a query says 1 the
entry runs (and computes the right thing), where it says 0 the entry returns VM_E_INVALID on the
host, before any launch, and writes nothing."""

import pytest
import torch
import torch.nn.functional as F

from videomamba_amd import _lib
from videomamba_amd import kernels as K
from videomamba_amd import options

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(autouse=True, scope="module")
def _gpu():
    assert torch.cuda.is_available(), "gpu-marked tests need a HIP device"


def _rows(m, cols, ld, off, scale=1.0):
    """(m, cols) bf16 rows of stride ``ld`` starting ``off`` elements into a fresh buffer."""
    buf = (torch.randn(m * ld + 16, device=DEV) * scale).to(BF)
    return buf.as_strided((m, cols), (ld, 1), off)


@pytest.mark.parametrize("n,k", [(192, 192), (200, 192), (100, 192), (192, 256)])
def test_linear_fits_agrees_with_vm_linear_fwd(n, k):
    """m 1 and 129 (two row tiles), row strides k, k + 8 and k + 4, x at a 16-byte aligned
    address and 8 bytes past one.  fits 1: VM_OK and the result within the bound
    tests/test_gpu_parity.py holds K.linear to (one bf16 rounding of an fp32 reference);
    fits 0: VM_E_INVALID and the NaN-filled output untouched."""
    lib = _lib.load()
    torch.manual_seed(n + k)
    w = (torch.randn(n, k, device=DEV) * k ** -0.5).to(BF)
    stream = torch.cuda.current_stream().cuda_stream
    seen = set()
    for m in (1, 129):
        for ldx in (k, k + 8, k + 4):
            for off in (0, 4):
                x = _rows(m, k, ldx, off)
                out = torch.full((m, n), float("nan"), device=DEV, dtype=BF)
                fits = K.linear_fits(m, n, k, ldx, k, n, x.data_ptr(), w.data_ptr(),
                                     out.data_ptr())
                rc = lib.vm_linear_fwd(x.data_ptr(), ldx, w.data_ptr(), k, None, out.data_ptr(),
                                       n, m, n, k, _lib.VM_DTYPE_BF16, stream)
                torch.cuda.synchronize()
                seen.add(fits)
                if fits:
                    assert rc == 0, (m, ldx, off, lib.vm_last_error())
                    ref = F.linear(x.float(), w.float())
                    assert ((out.float() - ref).abs() <= ref.abs() * 2.0 ** -8 + 1e-3).all()
                else:
                    assert rc == -1, (m, ldx, off)
                    assert torch.isnan(out).all()
                assert fits == (n % 8 == 0 and k == 192 and ldx % 8 == 0 and off == 0)
    assert seen == ({True, False} if (n, k) in ((192, 192), (200, 192)) else {False})


@pytest.mark.parametrize("ldh", [192, 384, 194])
def test_linear_add_norm_fits_agrees_with_the_entry(ldh):
    """m = 129, n = 192, k = 384 (a 2 x 3 grid: the one-launch form on any device) with hn
    contiguous, hn a column slice of a wider buffer (ldh = 2 n: taken), and a row stride the
    entry refuses (ldh % 4).  fits 1: bit-equal to vm_linear_fwd then vm_add_norm_fwd; fits 0:
    VM_E_INVALID, h / residual / hn untouched."""
    m, n, k = 129, 192, 384
    torch.manual_seed(ldh)
    x = torch.randn(m, k, device=DEV).to(BF)
    w = (torch.randn(n, k, device=DEV) * k ** -0.5).to(BF)
    res0 = torch.randn(m, n, device=DEV)
    nw = torch.rand(n, device=DEV) + 0.5
    res = res0.clone()
    hn = torch.full((m, ldh), float("nan"), device=DEV, dtype=BF)[:, :n]
    fits = K.linear_add_norm_fits(m, n, k, k, k, n, n, ldh,
                                  (x.data_ptr(), w.data_ptr(), 0, res.data_ptr(), nw.data_ptr(),
                                   hn.data_ptr()))
    assert fits == (ldh % 4 == 0)
    if not fits:
        with pytest.raises(RuntimeError, match="rc=-1"):
            K.linear_add_norm(x, w, res, nw, 1e-5, hn)
        torch.cuda.synchronize()
        assert torch.equal(res, res0) and torch.isnan(hn).all()
        return
    h = K.linear_add_norm(x, w, res, nw, 1e-5, hn)
    h_ref = K.linear(x, w)
    res_ref = res0.clone()
    hn_ref = torch.empty(m, n, device=DEV, dtype=BF)
    K.add_norm_raw(h_ref, res_ref, nw, None, hn_ref, res_ref, m, n, 1e-5, True,
                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(h, h_ref) and torch.equal(res, res_ref) and torch.equal(hn, hn_ref)


def _dtproj_call(Bz, D, L, R, segments):
    """vm_selective_scan_dtproj_fwd on random operands in the mixer's layout; returns the
    NaN-prefilled output (Bz, Lp, D), or the RuntimeError the entry's refusal raised."""
    N, E, Lp = 16, R + 32, (L + 7) // 8 * 8
    g = lambda *s: torch.randn(*s, device=DEV)  # noqa: E731
    U, XZ, XD = g(Bz * Lp, D).to(BF), g(Bz * Lp, 2 * D).to(BF), g(Bz * Lp, E).to(BF)
    wpad = torch.zeros(D, 32 if R <= 32 else 64, device=DEV, dtype=BF)
    wpad[:, :R] = (g(D, R) / R ** 0.5).to(BF)
    A = -torch.exp(g(D, N) * 0.1).contiguous()
    Dv, bias = g(D), g(D) * 0.5 - 2.0
    h = g(Bz, D, N).contiguous()
    y = torch.full((Bz * Lp, D), float("nan"), device=DEV, dtype=BF)
    s_u, s_z, s_bc = (Lp * D, 1, D), (Lp * 2 * D, 1, 2 * D), (Lp * E, 1, E)
    try:
        with options.override(scan_segments=segments):
            K.scan_dtproj_raw(U, s_u, XD, (Lp * E, E), R, wpad, A, XD[:, R:R + N], s_bc,
                              XD[:, R + N:], s_bc, Dv, XZ[:, D:], s_z, bias, h, (D * N, N), h,
                              (D * N, N), y, s_u, Lp, Bz, D, L, N,
                              torch.cuda.current_stream().cuda_stream)
    except RuntimeError as exc:
        torch.cuda.synchronize()
        assert torch.isnan(y).all()  # refused on the host: nothing written
        return exc
    torch.cuda.synchronize()
    return y.view(Bz, Lp, D)


@pytest.mark.parametrize("L,R,segments,want", [
    (64, 4, 1, 1), (200, 4, 1, 1),        # the single pass
    (64, 4, 8, 3), (200, 4, 25, 3),       # segmented: 2 and 8 workgroups, resident
    (200, 4, 2, 0),                       # 100-step segments: past the 64 the LDS dt block holds
    (64, 4, 0, None), (200, 4, 0, None),  # the cost model's count: whatever it is, they agree
    (64, 6, 1, 0), (200, 6, 25, 0),       # dt_rank no multiple of 4: both forms refuse
])
def test_scan_dtproj_fits_agrees_with_the_entry(L, R, segments, want):
    """B = 1, D = 128 (one workgroup of the single pass, two 64-channel groups of the chunked
    form), N = 16.  Answer 0: the entry refuses; 1 / 2 / 3: it runs, every step's output
    finite and the padded rows zero.  The segmented grids here are far below any CU count, so
    the device answers 3; answer 2 is the same call planned for fewer CUs than workgroups
    (``cus``), which the entry also takes."""
    Bz, D = 1, 128
    fits = K.scan_dtproj_fits(Bz, D, L, 16, R, segments)
    if want is not None:
        assert fits == want
    got = _dtproj_call(Bz, D, L, R, segments)
    if fits == 0:
        assert isinstance(got, RuntimeError) and "rc=-1" in str(got)
        return
    assert not isinstance(got, RuntimeError), got
    assert torch.isfinite(got[:, :L].float()).all() and not got[:, L:].float().abs().any()
    if fits >= 2:
        steps = K.scan_chunk_steps(Bz, D, L, 16, segments)
        segs = -(-L // steps)
        wgs = Bz * (D // 64) * -(-segs // 8)  # rows x channel groups x blocks of 8 segments
        assert wgs <= torch.cuda.get_device_properties(0).multi_processor_count and fits == 3
        assert K.scan_dtproj_fits(Bz, D, L, 16, R, segments, cus=wgs) == 3
        if wgs > 1:
            assert K.scan_dtproj_fits(Bz, D, L, 16, R, segments, cus=wgs - 1) == 2
    else:
        assert K.scan_dtproj_fits(Bz, D, L, 16, R, segments, cus=1) == 1
