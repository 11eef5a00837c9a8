"""CPU tests of the paired selective scan backward's host side (ABI v19): the new header
``include/videomamba_hip_ext.h`` against ``_lib._SIGNATURES_EXT`` argument by argument, the
new symbol in the library, every refusal of ``vm_selective_scan_bidir_bwd`` (no launch
happens: there is no GPU here), the option that selects the refiner's training path, and the
GPU test's float64 reference obtained two ways."""

import ctypes
import os
import re

import pytest
import torch

import scan_bidir_bwd_ref as pbr
import scan_matrix as sm
from videomamba_amd import _lib, options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = b"vm_selective_scan_bidir_bwd"
F32 = torch.float32


# ------------------------------------------------------------------ header and binding
def test_ext_header_matches_the_ctypes_table():
    """Every prototype of videomamba_hip_ext.h against ``_SIGNATURES_EXT`` (the parser of
    test_api_cpu: a declarator it does not know fails, it is not skipped), every symbol in the
    library, and the v18 table left alone."""
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 19 and lib.vm_abi_version() == _lib.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "videomamba_hip_ext.h")).read()
    assert '#include "videomamba_hip.h"' in header and "added after ABI v18" in header
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    code = re.sub(r"//[^\n]*", " ", code)
    code = "\n".join(ln for ln in code.splitlines() if not ln.lstrip().startswith("#"))
    scalars = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float,
               "vm_stream_t": ctypes.c_void_p}
    returns = {**scalars, "const char*": ctypes.c_char_p}

    def ctype(decl):
        m = re.fullmatch(r"(?:const\s+)?(\w+(?:\s+\w+)*?)\s*(\*?)\s*(\w+)", " ".join(decl.split()))
        assert m, f"unparsed declarator {decl!r}"
        return ctypes.c_void_p if m.group(2) else scalars[m.group(1)]

    protos = re.findall(r"([\w ]+?\*?)\s*\b(vm_\w+)\s*\(([^)]*)\)\s*;", code)
    parsed = {name: ([ctype(p) for p in params.split(",")], returns[" ".join(ret.split())])
              for ret, name, params in protos}
    assert len(parsed) == len(protos) == len(_lib.EXPORTED_EXT)
    assert set(parsed) == set(_lib.EXPORTED_EXT) == {"vm_selective_scan_bidir_bwd"}
    assert "vm_" not in re.sub(r"\bvm_\w+\s*\([^)]*\)\s*;|\bvm_stream_t\b", "", code), \
        "a vm_ declaration the prototype pattern did not take"
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, want in parsed.items():
        assert (list(_lib._SIGNATURES_EXT[name][0]), _lib._SIGNATURES_EXT[name][1]) == want, name
        assert getattr(raw, name) is not None
        assert getattr(lib, name).argtypes == _lib._SIGNATURES_EXT[name][0]  # load() bound it
        assert name not in _lib._SIGNATURES and name not in _lib.EXPORTED
    # the paired entry takes the plain entry's arguments up to dtype, then eleven of its own
    plain = _lib._SIGNATURES["vm_selective_scan_bwd"][0]
    ext = _lib._SIGNATURES_EXT["vm_selective_scan_bidir_bwd"][0]
    assert ext[:len(plain) - 3] == plain[:-3] and len(ext) == len(plain) + 11


def test_train_refiner_option_is_validated():
    assert options.Options().train_refiner in ("paired", "blocks")
    for v in ("paired", "blocks"):
        with options.override(train_refiner=v) as o:
            assert o.train_refiner == v
    with pytest.raises(ValueError, match="train_refiner"):
        with options.override(train_refiner="both"):
            pass


# ------------------------------------------------------------------ refusals
def _args(lib, ptr, *, split=2, batch=None, shape=(136, 24), sd=1, dstate=16, dtype=0,
          ws_short=0, frame=1, absent=()):
    """vm_selective_scan_bidir_bwd arguments of a token-major fp32 case of 2 split rows whose
    every pointer is ``ptr`` (never dereferenced: each call here is refused before any
    launch).  ``absent`` names backward-direction operands passed as NULL (with their
    gradient)."""
    D, L = shape
    Bz = 2 * split if batch is None else batch
    x = (ptr, L * D, sd, D)
    bc = (ptr, L * 16, 1, 16)
    st = (ptr, D * 16, 16)
    need = lib.vm_selective_scan_bwd_workspace_bytes(Bz, D, L, 16)
    b = lambda k: None if k in absent else ptr  # noqa: E731
    return [*x, *x, ptr, *bc, *bc, ptr, *x, ptr, 1, ptr, 0, D * 16, 16,  # inputs .. h0
            *x, *st,                                                    # dout, dh_last
            *x, *x, *x, *bc, *bc, ptr, ptr, ptr, *st,                   # gradients
            Bz, D, L, dstate, dtype,
            split, b("A"), b("D"), b("bias"), b("h0"), ptr,             # the backward direction
            b("dA"), b("D"), b("bias"), b("h0"), frame,
            ptr, need - ws_short, None]


def test_bidir_bwd_entry_refuses_bad_arguments_without_gpu():
    lib = _lib.load()
    fn = lib.vm_selective_scan_bidir_bwd
    host = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(host)
    assert len(_args(lib, ptr)) == len(_lib._SIGNATURES_EXT["vm_selective_scan_bidir_bwd"][0])
    null = _args(lib, None)
    cases = {
        "all-null": (null, b"null required pointer"),
        "A_bwd null": (_args(lib, ptr, absent=("A",)), b"null required pointer"),
        "dA_bwd null": (_args(lib, ptr, absent=("dA",)), b"null required pointer"),
        "batch 5, split 2": (_args(lib, ptr, batch=5), b"must be 2*split"),
        "batch 2, split 2": (_args(lib, ptr, batch=2), b"must be 2*split"),
        "dstate 8": (_args(lib, ptr, dstate=8), b"dstate must be 16"),
        "channel stride": (_args(lib, ptr, sd=2), b"token-major operands only"),
        "frame_len 0": (_args(lib, ptr, frame=0), b"frame_len=0"),
        "frame_len 5 of 24": (_args(lib, ptr, frame=5), b"frame_len=5"),
        "short workspace": (_args(lib, ptr, ws_short=1), b"workspace of"),
        "D one-sided": (_args(lib, ptr, absent=("D",)), b"both directions"),
        "bias one-sided": (_args(lib, ptr, absent=("bias",)), b"both directions"),
        "h0 one-sided": (_args(lib, ptr, absent=("h0",)), b"both directions"),
        "dtype": (_args(lib, ptr, dtype=7), b"unsupported dtype"),
    }
    for what, (args, msg) in cases.items():
        # another entry's message is in place first
        lib.vm_add_norm_fwd(None, 0, None, 0, None, None, None, 0, None, 0, 1, 8, 1e-5, 1, None)
        assert ENTRY not in lib.vm_last_error()
        assert fn(*args) == -1, what
        err = lib.vm_last_error()
        assert ENTRY in err and msg in err, (what, err)
    # frame_len 4 divides 24 and split 0 is a batch of 0: neither is a refusal by itself
    ok = _args(lib, ptr, frame=4, ws_short=1)
    assert fn(*ok) == -1 and b"workspace of" in lib.vm_last_error()


# ------------------------------------------------------------------ the GPU test's reference
@pytest.mark.parametrize("F", [1, 4])
def test_paired_reference_two_ways(F):
    """Side A (grads64 per half, the backward half's dout gathered through pair_out_row)
    against side B (float64 autograd through the paired forward restated with a row scatter):
    2 + 2 rows of (5, 12, 16), everything present, to 1e-12."""
    row = sm.ROWS[1]
    split, D, L, N = 2, 5, 12, 16
    pi = sm.make_pair_inputs(row, F32, split, D, L, N, seed=1)
    dout, dhl, dhl_b = pbr.make_dout(row, F32, split, D, L, N)
    assert dout.shape == (2 * split, D, L) and dhl.shape == dhl_b.shape == (split, D, N)
    a = pbr.grads64_paired(pi, row, dout, dhl, dhl_b, F)
    b = pbr.grads64_paired_autograd(pi, row, dout, dhl, dhl_b, F)
    assert set(a) == set(b) == set(pbr.NAMES)
    for k in pbr.NAMES:
        assert a[k].dtype == torch.float64 and a[k].shape == b[k].shape
        scale = float(a[k].abs().max())
        assert scale > 0
        assert float((a[k] - b[k]).abs().max()) <= 1e-12 * max(1.0, scale), k
    # the restated forward is the forward matrix's paired reference
    y_ref, hf_ref, hb_ref = pi.ref(row.softplus, F)
    f, r = pbr.halves(pi)
    y_r, _ = r.ref(row.softplus)
    idx = pbr.out_rows(L, F)
    assert sorted(idx.tolist()) == list(range(L))
    torch.testing.assert_close(y_ref[split:][:, :, idx], y_r, rtol=0, atol=0)
    # and the gather is not the identity: the reference would notice a kernel that skips it
    assert idx.tolist() != list(range(L))
    assert not torch.equal(pbr.flipped_dout(dout, split, F), dout[split:])
