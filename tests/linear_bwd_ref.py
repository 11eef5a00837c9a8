"""Projection GEMM backward: seeded inputs, float64 references and the case lists that
``test_linear_bwd_cpu.py`` (no GPU) and ``test_gpu_linear_bwd.py`` share.  A helper module,
not a conftest: it defines no fixtures and no hooks.

Reference
    ``dw = dy^T x`` and ``dx = dy w`` as float64 matmuls of the bf16 operands (exact
    products, so the reference's own error is float64 rounding of the sum).  References are
    computed once per case and cached; callers must not modify them.

Comparator
    ``train_bwd_ref.assert_within_rms``: ``|got - ref| <= tol (rms(ref) + |ref|)``, tol 1e-4
    for values stored in fp32 and 2e-2 for values stored in bf16 against the reference
    rounded once to bf16.

Cases
    Raw wgrad: m in {1, 65, S + 1, 3 S + 5} with S = 256, the plan's slice rows at these m
    (``vm_linear_wgrad_slice_rows``; asserted in test_linear_bwd_cpu.py): one short slice, a
    row-block tail, a one-row second slice, four slices with a tail.  n in {8, 72, 192, 2304}:
    below a tile, a tile tail, one tile and a half, VideoMamba-M's in_proj.  k in {64, 192,
    576, 1152}.  dw in fp32 and bf16.  The product is thinned by cycling k and the dw dtype
    along (m, n), with every value of every axis present.
"""

from __future__ import annotations

import functools
import itertools

import torch

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64

S = 256  # kWgMinSliceRows (csrc/vm_gemm_wgrad_plan.h): the slice rows of every m used here
WG_M = (1, 65, S + 1, 3 * S + 5)
WG_N = (8, 72, 192, 2304)
WG_K = (64, 192, 576, 1152)
WG_DT = (F32, BF16)


def wgrad_cases():
    """(m, n, k, dw dtype, strided): the thinned product, VideoMamba-M's two projections in the
    other dw dtype, and one case on column-sliced views (lddy > n, ldx > k, lddw > k)."""
    out = []
    for (i, m), (j, n) in itertools.product(enumerate(WG_M), enumerate(WG_N)):
        out.append((m, n, WG_K[(i + j) % 4], WG_DT[(i + j // 2) % 2], False))
    out += [(3 * S + 5, 2304, 576, BF16, False), (S + 1, 576, 1152, F32, False),
            (S + 1, 72, 192, BF16, True)]
    return out


DG_NK = ((768, 192), (192, 384), (2304, 576), (576, 1152))
DG_M = (1, 129, 300)
FWD_K = (192, 384, 576, 768, 1152, 1536)  # vm_linear_fwd's reduction lengths


def _randn_bf16(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(BF16)


@functools.lru_cache(maxsize=None)
def wgrad_inputs(m, n, k):
    """dy (m, n), x (m, k): seeded randn cast to bf16, on the CPU."""
    return _randn_bf16((m, n), 1000 + m + n), _randn_bf16((m, k), 2000 + m + k)


@functools.lru_cache(maxsize=None)
def wgrad_ref64(m, n, k):
    dy, x = wgrad_inputs(m, n, k)
    return dy.to(F64).t() @ x.to(F64)


@functools.lru_cache(maxsize=None)
def dgrad_inputs(m, n, k):
    """dy (m, n), w (n, k) with entries of variance 1 / n so dx has unit scale."""
    return _randn_bf16((m, n), 3000 + m + n), (_randn_bf16((n, k), 4000 + n + k).float()
                                                * n ** -0.5).to(BF16)


@functools.lru_cache(maxsize=None)
def dgrad_ref64(m, n, k):
    dy, w = dgrad_inputs(m, n, k)
    return dy.to(F64) @ w.to(F64)


def stored_ref(ref64, stored):
    """(tolerance, reference rounded once to the storage dtype, as fp32)."""
    return {F32: 1e-4, BF16: 2e-2}[stored], ref64.to(stored).to(F32)
