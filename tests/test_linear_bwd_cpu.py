"""Projection GEMM backward (ABI v17) without a GPU: the exported symbols, the workspace
query against the header's bound, every refusal of ``vm_linear_wgrad`` / ``vm_linear_dgrad``
(refused before any launch: the pointers are null or host memory), the host plan walked by a
stand-alone sanitizer build, and the inputs of test_gpu_linear_bwd.py: an fp32 matmul of the
same bf16 operands — fp32 accumulation in another order — sits inside the fp32 bound for
every case, so a failing GPU case points at the kernel and not at the inputs.
"""

import ctypes
import os
import shutil
import subprocess

import pytest
import torch

import linear_bwd_ref as lbr
import train_bwd_ref as tbr
from videomamba_amd import _lib, options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WGRAD, DGRAD = b"vm_linear_wgrad", b"vm_linear_dgrad"
F32, BF16 = torch.float32, torch.bfloat16


def test_abi_v17_symbols_load():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 17 and lib.vm_abi_version() == _lib.ABI_VERSION
    for name in ("vm_linear_wgrad", "vm_linear_wgrad_workspace_bytes", "vm_linear_dgrad"):
        assert name in _lib.EXPORTED
        assert getattr(ctypes.CDLL(_lib.LIB_PATH), name) is not None


def test_wgrad_workspace_query_is_monotone_and_bounded():
    """4 n k min(max_slices, ceil(m / 256)) bytes, never shrinking as m grows and at most
    16 n k + 32 MiB (the header's bound) for any m; pure host code."""
    q = _lib.load().vm_linear_wgrad_workspace_bytes
    ms = (0, 1, 255, 256, 257, 773, 1024, 1025, 1537, 3144, 12552, 50208, 10 ** 6)
    for n in (8, 72, 192, 576, 2304):
        for k in (64, 192, 576, 1152, 2304):
            prev = 0
            for m in ms:
                got = q(m, n, k)
                assert prev <= got <= 16 * n * k + (32 << 20), (m, n, k, got)
                assert got % (4 * n * k) == 0
                prev = got
            assert q(0, n, k) == 0 and q(1, n, k) == 4 * n * k and q(257, n, k) == 8 * n * k
            assert q(10 ** 6, n, k) == q(10 ** 7, n, k)  # capped
    # VideoMamba-M at B = 8 and 32: 5 and 11 slices
    assert q(12552, 2304, 576) == q(50208, 2304, 576) == 5 * 4 * 2304 * 576
    assert q(12552, 576, 1152) == q(50208, 576, 1152) == 11 * 4 * 576 * 1152


def test_gpu_cases_use_the_plans_slice_rows_and_cover_every_axis():
    rows = _lib.load().vm_linear_wgrad_slice_rows
    cases = lbr.wgrad_cases()
    for m, n, k, _, _ in cases:
        assert rows(m, n, k) == lbr.S, (m, n, k)
    assert {c[0] for c in cases} == set(lbr.WG_M) and {c[1] for c in cases} >= set(lbr.WG_N)
    assert {c[2] for c in cases} == set(lbr.WG_K) and {c[3] for c in cases} == set(lbr.WG_DT)
    for dt in lbr.WG_DT:
        sub = [c for c in cases if c[3] == dt]
        assert {c[0] for c in sub} == set(lbr.WG_M) and {c[1] for c in sub} >= set(lbr.WG_N)
    assert sum(c[4] for c in cases) == 1
    assert (3 * lbr.S + 5, 2304, 576) in {c[:3] for c in cases}


def test_fp32_matmul_of_the_inputs_sits_inside_the_fp32_bound():
    """The inputs of every GPU case: an fp32 CPU matmul of the same bf16 operands against the
    float64 reference, held to the bound of a value stored in fp32."""
    worst = 0.0
    for m, n, k in sorted({c[:3] for c in lbr.wgrad_cases()}):
        dy, x = lbr.wgrad_inputs(m, n, k)
        tol, ref = lbr.stored_ref(lbr.wgrad_ref64(m, n, k), F32)
        worst = max(worst, tbr.assert_within_rms(dy.float().t() @ x.float(), ref, tol,
                                                 f"dw {m} {n} {k}"))
    for (n, k), m in [(nk, m) for nk in lbr.DG_NK for m in lbr.DG_M]:
        dy, w = lbr.dgrad_inputs(m, n, k)
        tol, ref = lbr.stored_ref(lbr.dgrad_ref64(m, n, k), F32)
        worst = max(worst, tbr.assert_within_rms(dy.float() @ w.float(), ref, tol,
                                                 f"dx {m} {n} {k}"))
    print(f"\nfp32 matmul vs float64, worst ratio {worst:.4f}")


def _wgrad_args(lib, ptr, *, m=257, n=72, k=192, lddy=None, ldx=None, lddw=None, dw_dtype=0,
                dtype=1, ws_short=0, ptrs=None):
    need = lib.vm_linear_wgrad_workspace_bytes(m, n, k)
    p = dict(dy=ptr, x=ptr, dw=ptr, ws=ptr)
    p.update(ptrs or {})
    return [p["dy"], n if lddy is None else lddy, p["x"], k if ldx is None else ldx, p["dw"],
            k if lddw is None else lddw, dw_dtype, m, n, k, dtype, p["ws"], need - ws_short, None]


def _dgrad_args(ptr, *, m=129, n=768, k=192, lddy=None, ldwT=None, lddx=None, dtype=1, ptrs=None):
    p = dict(dy=ptr, wT=ptr, dx=ptr)
    p.update(ptrs or {})
    return [p["dy"], n if lddy is None else lddy, p["wT"], n if ldwT is None else ldwT, p["dx"],
            k if lddx is None else lddx, m, n, k, dtype, None]


def _other_entrys_message(lib):
    lib.vm_add_norm_fwd(None, 0, None, 0, None, None, None, 0, None, 0, 4, 64, 1e-5, 1, None)
    assert b"vm_add_norm_fwd" in lib.vm_last_error()


def test_wgrad_entry_refuses_bad_arguments_without_gpu():
    lib = _lib.load()
    host = ctypes.create_string_buffer(256)
    ptr = (ctypes.addressof(host) + 15) // 16 * 16
    assert len(_wgrad_args(lib, ptr)) == len(_lib._SIGNATURES["vm_linear_wgrad"][0])
    null = _wgrad_args(lib, None)
    null[-3:] = [None, 0, None]
    cases = {
        "all-null": null,
        "fp32 operands": _wgrad_args(lib, ptr, dtype=0),
        "dtype": _wgrad_args(lib, ptr, dtype=7),
        "dw dtype": _wgrad_args(lib, ptr, dw_dtype=7),
        "n % 8": _wgrad_args(lib, ptr, n=76),
        "k % 64": _wgrad_args(lib, ptr, k=96),
        "negative m": _wgrad_args(lib, ptr, m=-1),
        "lddy below n": _wgrad_args(lib, ptr, lddy=64),
        "ldx below k": _wgrad_args(lib, ptr, ldx=128),
        "lddw below k": _wgrad_args(lib, ptr, lddw=128),
        "lddy % 8": _wgrad_args(lib, ptr, lddy=76),
        "ldx % 8": _wgrad_args(lib, ptr, ldx=196),
        "lddw % 8": _wgrad_args(lib, ptr, lddw=196),
        "misaligned dy": _wgrad_args(lib, ptr, ptrs=dict(dy=ptr + 2)),
        "misaligned x": _wgrad_args(lib, ptr, ptrs=dict(x=ptr + 8)),
        "misaligned dw": _wgrad_args(lib, ptr, ptrs=dict(dw=ptr + 4)),
        "misaligned workspace": _wgrad_args(lib, ptr, ptrs=dict(ws=ptr + 8)),
        "dy past 2 GB": _wgrad_args(lib, ptr, m=50208, lddy=21504),
        "x past 2 GB": _wgrad_args(lib, ptr, m=50208, ldx=21504),
        "short workspace": _wgrad_args(lib, ptr, ws_short=1),
        "no workspace": _wgrad_args(lib, ptr, ptrs=dict(ws=None)),
        "null dw at m = 0": _wgrad_args(lib, ptr, m=0, ptrs=dict(dw=None)),
    }
    for what, args in cases.items():
        _other_entrys_message(lib)
        assert WGRAD not in lib.vm_last_error()
        assert lib.vm_linear_wgrad(*args) == -1, what
        assert WGRAD in lib.vm_last_error(), (what, lib.vm_last_error())
    for null_one in ("dy", "x", "dw"):
        args = _wgrad_args(lib, ptr, ptrs={null_one: None})
        assert lib.vm_linear_wgrad(*args) == -1 and WGRAD in lib.vm_last_error(), null_one


def test_dgrad_entry_refuses_bad_arguments_without_gpu():
    lib = _lib.load()
    host = ctypes.create_string_buffer(256)
    ptr = (ctypes.addressof(host) + 15) // 16 * 16
    assert len(_dgrad_args(ptr)) == len(_lib._SIGNATURES["vm_linear_dgrad"][0])
    cases = {
        "all-null": _dgrad_args(None),
        "null dy": _dgrad_args(ptr, ptrs=dict(dy=None)),
        "null wT": _dgrad_args(ptr, ptrs=dict(wT=None)),
        "null dx": _dgrad_args(ptr, ptrs=dict(dx=None)),
        "fp32": _dgrad_args(ptr, dtype=0),
        "n outside the list": _dgrad_args(ptr, n=640),
        "n 64": _dgrad_args(ptr, n=64),
        "n % 64": _dgrad_args(ptr, n=200),
        "k % 8": _dgrad_args(ptr, k=100),
        "lddy below n": _dgrad_args(ptr, lddy=512),
        "ldwT below n": _dgrad_args(ptr, ldwT=512),
        "lddx below k": _dgrad_args(ptr, lddx=128),
        "lddy % 8": _dgrad_args(ptr, lddy=772),
        "misaligned dy": _dgrad_args(ptr, ptrs=dict(dy=ptr + 2)),
        "misaligned wT": _dgrad_args(ptr, ptrs=dict(wT=ptr + 8)),
        "misaligned dx": _dgrad_args(ptr, ptrs=dict(dx=ptr + 4)),
        "negative m": _dgrad_args(ptr, m=-1),
    }
    for what, args in cases.items():
        _other_entrys_message(lib)
        assert DGRAD not in lib.vm_last_error()
        assert lib.vm_linear_dgrad(*args) == -1, what
        assert DGRAD in lib.vm_last_error(), (what, lib.vm_last_error())
    # 36 K steps are the dgrad's alone: the forward still refuses k = 2304
    assert lib.vm_linear_fwd(ptr, 2304, ptr, 2304, None, ptr, 576, -1, 576, 2304, 1, None) == -1
    fwd = [ptr, 2304, ptr, 2304, None, ptr, 576, 0, 576, 2304, 1, None]
    assert lib.vm_linear_fwd(*fwd) == -1 and b"k = 2304" in lib.vm_last_error()
    # and m == 0 is VM_OK for both new entries' accepted shapes (nothing launches)
    assert lib.vm_linear_dgrad(*_dgrad_args(ptr, m=0, n=2304, k=576)) == 0


def test_linear_fn_fits_takes_the_reduction_lengths_the_entries_take():
    """``kernels.linear_fn_fits`` decides what ``linear_fn`` sends to the HIP GEMMs, from the
    entries' own plans: its k are the reduction lengths ``vm_linear_fwd`` accepts and its n
    those ``vm_linear_dgrad`` accepts (an m = 0 call is VM_OK exactly for a reduction length
    of the list; nothing launches)."""
    from videomamba_amd import kernels as K
    lib = _lib.load()
    host = ctypes.create_string_buffer(256)
    ptr = (ctypes.addressof(host) + 15) // 16 * 16
    taken = tuple(n for n in range(64, 4097, 64)
                  if lib.vm_linear_dgrad(*_dgrad_args(ptr, m=0, n=n, k=192)) == 0)
    assert taken == (192, 384, 576, 768, 1152, 1536, 2304)
    fwd = tuple(k for k in range(64, 4097, 64)
                if lib.vm_linear_fwd(ptr, k, ptr, k, None, ptr, 192, 0, 192, k, 1, None) == 0)
    assert fwd == taken[:-1]  # the forward did not widen
    assert tuple(n for n in range(64, 4097, 64) if K.linear_fn_fits(129, n, 192)) == taken
    assert tuple(k for k in range(64, 4097, 64) if K.linear_fn_fits(129, 192, k)) == fwd


def test_train_gemm_option_is_validated():
    assert options.Options().train_gemm in ("hip", "library")
    with options.override(train_gemm="library") as o:
        assert o.train_gemm == "library"
    with options.override(train_gemm="hip") as o:
        assert o.train_gemm == "hip"
    with pytest.raises(ValueError, match="train_gemm"):
        with options.override(train_gemm="torch"):
            pass


def test_linear_fn_takes_the_library_path_on_the_cpu():
    """CPU operands never reach a HIP kernel: ``linear_fn`` is ``F.linear`` there, under
    either option."""
    from videomamba_amd import kernels as K
    x = torch.randn(3, 5, 192, dtype=BF16).requires_grad_(True)
    w = torch.randn(384, 192, dtype=BF16).requires_grad_(True)
    for mode in ("hip", "library"):
        with options.override(train_gemm=mode):
            y = K.linear_fn(x, w)
        assert torch.equal(y, torch.nn.functional.linear(x, w))
        assert y.grad_fn is not None and type(y.grad_fn).__name__ != "_LinearBackward"


def test_wgrad_plan_check_program_passes_under_sanitizers(tmp_path):
    """tests/host/gemm_wgrad_plan_check.cpp walks plan_linear_wgrad over a grid of (m, n, k)
    and exits non-zero unless the slices tile [0, m) and the tiles (n, k) exactly once, the
    workspace equals the query and respects the bound, and the refusals come in order.  A
    program of its own built with the host compiler under ASan + UBSan; nothing is loaded
    into Python."""
    name = "gemm_wgrad_plan_check"
    rocm_clang = "/opt/rocm/llvm/bin/clang++"
    cxx = [rocm_clang] if os.path.exists(rocm_clang) else \
        [shutil.which("g++") or "g++", "-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / name)
    subprocess.run(cxx + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "videomamba_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", name + ".cpp"), "-o", exe],
                   check=True, timeout=120)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout
