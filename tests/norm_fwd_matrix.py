"""Norm forward, norm + pool and one-token step matrix: the float64 references, the seeded
inputs, the case tables and the host dispatch restated, which ``test_norm_fwd_matrix_cpu.py``
(no GPU) and ``test_gpu_norm_fwd_matrix.py`` share.  A helper module, not a conftest: it
defines no fixtures and no hooks.

References (float64 on the stored input values; bf16 inputs are upcast, never re-rounded)
    add + norm      ``train_bwd_ref.add_norm_fwd64``; ``residual_out`` is exact: the one
                    correctly rounded fp32 add ``x.float() + residual.float()``, rounded once
                    more where it is stored in bf16 (:func:`sum_exact`).
    norm + pool     :func:`norm_pool_ref64`: output row r of a batch row is the normalised input
                    row :func:`pool_row_map` names (``rev_frame`` reverses the frame order of
                    the grouped rows); :func:`slice_sums64` are the fp64 column sums of features
                    as they are stored, per (batch row, group, 16-row slice) — the workspace's
                    layout, zeros past a short group's end.
    pool finish     :func:`pool_finish_ref64`: the mean rounded to ``xp_dtype``, cls+avg rounded
                    again, cls_cat_avg with the CLS row first, then LayerNorm with nullable
                    weight and bias.
    one-token steps :func:`ssm_step_ref64` (the state read from its stored dtype; the output
                    uses the new state before it is rounded for the store, as the oracle does)
                    and :func:`conv_step_ref64` (the shifted state as stored, then the dot).

Dispatch
    :func:`add_norm_instance` and :func:`pool_instance` restate which kernel instance
    ``vm_add_norm_fwd`` / ``vm_norm_pool_fwd`` launch (``vm_norm_plan.h``: ``vec``, the fast
    path, ``cpl``, ``vpl``, write-through); ``ADD_NORM_INSTANCES`` (28) and ``POOL_INSTANCES`` (8)
    list every one, and the CPU test asserts the case tables reach them all.  The restatement is
    the tests' own; ``plan_line`` gives a case as ``tests/host/norm_fwd_instance_of.cpp`` reads
    it, and the CPU test holds every case's restated instance to the one the library's planner
    names (``SMALL_STORE_ROWS`` and ``POOL_RB`` to the header's values likewise).

Comparator
    ``train_bwd_ref.tol_and_ref`` / ``assert_within_rms``: ``|got - ref| <= tol (rms(ref) +
    |ref|)``, 1e-4 for values stored in fp32, 2e-2 for values stored in bf16 against the
    reference rounded once.

Sentinels
    :class:`Guarded` puts a tensor between two 4 KiB margins of a byte pattern (1024 fp32 or
    2048 bf16 elements each) and tells whether anything outside the region a launch may write
    has changed — the margins and, for a padded buffer, the padding rows and columns.
"""

from __future__ import annotations

import itertools
import math
from typing import Callable, List, NamedTuple, Optional, Tuple

import torch

import train_bwd_ref as tbr
from train_bwd_ref import assert_within_rms, tol_and_ref  # noqa: F401  (re-exported)

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
EPS = 1e-5
SMALL_STORE_ROWS = 32768   # kSmallStoreRows (vm_norm_plan.h): the write-through switch
POOL_RB = 16               # kPoolRB (vm_norm_plan.h): rows of one pooling slice
MARGIN = 4096              # sentinel bytes on either side of a guarded tensor

_name = lambda dt: {None: "none", F32: "fp32", BF16: "bf16", F64: "fp64"}[dt]  # noqa: E731
_other = lambda dt: BF16 if dt == F32 else F32  # noqa: E731
_code = lambda dt: 1 if dt == BF16 else 0  # noqa: E731  (VM_DTYPE_BF16 / VM_DTYPE_F32)


def f64(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else t.detach().cpu().to(F64)


# --------------------------------------------------------------------------- sentinels
class Guarded:
    """A tensor of ``shape`` / ``dt`` inside a byte buffer with :data:`MARGIN` sentinel bytes
    on either side.  ``region`` maps the full tensor to the part a launch may write (default:
    all of it); ``t`` is that part, ``full`` the whole tensor.  :meth:`intact` is true while
    every byte outside the region still has the bits it had when :meth:`arm` was called (at
    construction, after ``fill`` is copied into the region)."""

    def __init__(self, shape, dt, device, region: Optional[Callable] = None, fill=None):
        self.shape, self.dt = tuple(shape), dt
        self.nbytes = math.prod(self.shape) * torch.empty((), dtype=dt).element_size()
        self.buf = torch.full((MARGIN + self.nbytes + MARGIN,), 0xA5, dtype=torch.uint8,
                              device=device)
        self.region = region or (lambda t: t)
        self.full = self._view(self.buf)
        self.t = self.region(self.full)
        if fill is not None:
            self.t.copy_(fill)
        self.arm()

    def _view(self, buf):
        return buf[MARGIN:MARGIN + self.nbytes].view(self.dt).view(self.shape)

    def _outside(self, buf):
        c = buf.clone()
        self.region(self._view(c)).zero_()
        return c

    def arm(self):
        self.snapshot = self.buf.clone()
        self.before = self._outside(self.buf)

    def intact(self) -> bool:
        return torch.equal(self.before, self._outside(self.buf))

    def unchanged(self) -> bool:
        """Nothing at all was written, the region included (a refused call)."""
        return torch.equal(self.snapshot, self.buf)


# --------------------------------------------------------------------------- add + norm
class NormCase(NamedTuple):
    """One ``vm_add_norm_fwd`` call.  ``ro``: "none", "fp32", "bf16" (a separate
    ``residual_out`` of that dtype) or "alias" (``residual_out`` is ``residual``).  ``offset``:
    elements by which ``x`` starts past a 16-byte boundary (a view into a larger buffer)."""
    rows: int
    cols: int
    rms: bool
    bias: bool
    x: torch.dtype
    out: torch.dtype
    res: Optional[torch.dtype]
    ro: str
    offset: int = 0

    @property
    def ro_dtype(self) -> Optional[torch.dtype]:
        return {"none": None, "fp32": F32, "bf16": BF16, "alias": self.res}[self.ro]

    @property
    def id(self) -> str:
        return (f"r{self.rows}-c{self.cols}-{'rms' if self.rms else 'ln'}"
                f"{'-bias' if self.bias else ''}-x{_name(self.x)}-y{_name(self.out)}-"
                f"res{_name(self.res)}-ro{self.ro}{'-off%d' % self.offset if self.offset else ''}")

    def plan_line(self) -> str:
        """The case as ``tests/host/norm_fwd_instance_of.cpp`` reads it (kind 1): rows, cols,
        is_rms, bias, x / out dtype codes, residual and residual_out presence and dtype codes,
        and whether ``x`` is 16-byte aligned (every other buffer is)."""
        rod = self.ro_dtype
        x_al = (self.offset * (2 if self.x == BF16 else 4)) % 16 == 0
        return " ".join(str(int(v)) for v in (
            1, self.rows, self.cols, self.rms, self.bias, _code(self.x), _code(self.out),
            self.res is not None, _code(self.res), rod is not None, _code(rod), x_al))


def add_norm_instance(c: NormCase) -> tuple:
    """The kernel instance ``vm_add_norm_fwd`` launches for this call: ("fast", CPL, RES, RO,
    write-through) for ``add_rms_bf16_kernel``, ("vec", CPL) for ``add_norm_vec_kernel``,
    ("scalar", VPL) for ``add_norm_kernel``.  Every buffer but ``x`` is 16-byte aligned."""
    rod = c.ro_dtype
    vec = c.cols % 4 == 0 and (c.offset * (2 if c.x == BF16 else 4)) % 16 == 0
    if (vec and c.rms and not c.bias and c.x == BF16 and c.out == BF16 and c.res in (None, F32)
            and rod in (None, F32) and c.cols <= 1024):
        res, ro = c.res is not None, rod is not None
        return ("fast", (c.cols + 255) // 256, res, ro,
                res and ro and c.rows <= SMALL_STORE_ROWS)
    if vec:
        cpl = (c.cols + 255) // 256
        return ("vec", 1 if cpl <= 1 else 2 if cpl <= 2 else 4 if cpl <= 4 else 8)
    vpl = (c.cols + 63) // 64
    return ("scalar", 4 if vpl <= 4 else 8 if vpl <= 8 else 16 if vpl <= 16 else 32)


ADD_NORM_INSTANCES = (
    [("fast", cpl, res, ro, False) for cpl in (1, 2, 3, 4) for res in (False, True)
     for ro in (False, True)] + [("fast", cpl, True, True, True) for cpl in (1, 2, 3, 4)]
    + [("vec", c) for c in (1, 2, 4, 8)] + [("scalar", v) for v in (4, 8, 16, 32)])

NORM_ROWS = (1, 3, 4, 5, 257)
COLS_VEC = (4, 8, 256, 260, 512, 516, 768, 772, 1024, 1028, 2048)
COLS_SCALAR = (1, 63, 65, 255, 257, 511, 513, 1023, 1025, 2047)
NORM_KINDS = ((True, False), (False, True), (False, False), (True, True))   # (rms, bias)
NORM_RES = (None, F32, BF16)
NORM_RO = ("none", "fp32", "bf16", "alias")
FAST_COLS = tuple(c for c in COLS_VEC if c <= 1024)
FAST_FORMS = ((None, "none"), (None, "fp32"), (F32, "none"), (F32, "fp32"), (F32, "alias"))
WT_PAIR = (SMALL_STORE_ROWS, SMALL_STORE_ROWS + 1)
# add_rms_bf16_kernel<CPL, true, true> without write-through needs more than kSmallStoreRows
# rows; CPL 2, 3 and 4 need 260, 516 and 772 columns at the least.  These three cases are the
# only ones above 32769 x 8 / 257 x 2048; their float64 reference runs on BIG_REF_ROWS rows.
BIG_COLS = (260, 516, 772)
BIG_REF_ROWS = 261
MISALIGNED = NormCase(5, 576, True, False, BF16, BF16, F32, "fp32", offset=1)


def _norm_cases() -> List[NormCase]:
    out = []
    # every (cols, rows) in both x dtypes, the other axes cycling along
    for j, (cols, rows) in enumerate(itertools.product(COLS_VEC + COLS_SCALAR, NORM_ROWS)):
        for o, xdt in enumerate((F32, BF16)):
            rms, bias = NORM_KINDS[(j + o) % 4]
            res = NORM_RES[(j + j // 3 + o) % 3]
            ro = NORM_RO[(j + j // 4 + 2 * o) % 4]
            if ro == "alias" and res is None:
                ro = "none"
            out.append(NormCase(rows, cols, rms, bias, xdt,
                                xdt if (j // 2 + o) % 2 == 0 else _other(xdt), res, ro))
    # the fast path: every CPL with every (residual, residual_out) form
    for j, (cols, (res, ro)) in enumerate(itertools.product(FAST_COLS, FAST_FORMS)):
        out.append(NormCase(NORM_ROWS[j % 5], cols, True, False, BF16, BF16, res, ro))
    # either side of the write-through switch, and the fast path's neighbours there
    for rows in WT_PAIR:
        out.append(NormCase(rows, 8, True, False, BF16, BF16, F32, "fp32"))
    out.append(NormCase(WT_PAIR[1], 8, False, True, F32, BF16, BF16, "alias"))
    out += [NormCase(WT_PAIR[1], cols, True, False, BF16, BF16, F32, "fp32") for cols in BIG_COLS]
    out.append(MISALIGNED)
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


NORM_CASES = _norm_cases()


def norm_ref_rows(c: NormCase) -> Optional[torch.Tensor]:
    """Row indices the float64 reference of a case runs on (None: all): the big cases keep
    their first and last rows, both sides of every workgroup's four."""
    if c.rows * c.cols <= 257 * 2048:
        return None
    half = BIG_REF_ROWS // 2
    return torch.cat([torch.arange(0, half), torch.arange(c.rows - (BIG_REF_ROWS - half), c.rows)])


def norm_inputs(c: NormCase, seed: int = 1):
    """Seeded CPU operands: x (rows, cols) in ``c.x``, residual in ``c.res`` or None, weight and
    bias (cols) fp32 — ``train_bwd_ref.norm_inputs``'s recipe without its gradients."""
    g = torch.Generator().manual_seed(seed + 7 * c.rows + c.cols)
    x = torch.randn(c.rows, c.cols, generator=g).to(c.x)
    res = (2.0 * torch.randn(c.rows, c.cols, generator=g)).to(c.res) if c.res is not None else None
    w = 1.0 + 0.2 * torch.randn(c.cols, generator=g)
    b = 0.2 * torch.randn(c.cols, generator=g) if c.bias else None
    return {"x": x, "residual": res, "weight": w, "bias": b}


def add_norm_ref64(ops, rms: bool, rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float64 y of the fused add + norm on the stored operands (``rows``: a subset)."""
    x, r = f64(ops["x"]), f64(ops["residual"])
    if rows is not None:
        x, r = x[rows], None if r is None else r[rows]
    return tbr.add_norm_fwd64(x, r, f64(ops["weight"]), f64(ops["bias"]), EPS, rms, False)


def sum_exact(x: torch.Tensor, res: Optional[torch.Tensor], stored: torch.dtype) -> torch.Tensor:
    """``residual_out``: one correctly rounded fp32 add, rounded once more to ``stored``."""
    s = x.float() if res is None else x.float() + res.float()
    return s.to(stored)


def layer_norm_ref64(v, weight, bias, eps):
    """LayerNorm of float64 rows with nullable weight and bias."""
    c = v - v.mean(-1, keepdim=True)
    y = c * torch.rsqrt(c.pow(2).mean(-1, keepdim=True) + eps)
    if weight is not None:
        y = y * weight
    if bias is not None:
        y = y + bias
    return y


# --------------------------------------------------------------------------- norm + pool
POOL_BATCH = 2


class PoolCase(NamedTuple):
    """One ``vm_norm_pool_fwd`` call over :data:`POOL_BATCH` batch rows.  ``sizes``: the group
    sizes of each batch row (equal sums); ``implicit``: the groups are passed as (groups,
    group_rows), every batch row alike, else as int32 ``bounds``; ``mgr``: max_group_rows."""
    cols: int
    x: torch.dtype
    out: torch.dtype
    res: Optional[torch.dtype]
    rms: bool
    bias: bool
    head: int
    sizes: Tuple[Tuple[int, ...], ...]
    implicit: bool
    mgr: int
    rev_frame: int
    sums: bool

    @property
    def groups(self) -> int:
        return len(self.sizes[0])

    @property
    def rows(self) -> int:
        return self.head + sum(self.sizes[0])

    @property
    def slices(self) -> int:
        return (self.mgr + POOL_RB - 1) // POOL_RB if self.mgr > 0 else 1

    def bounds(self) -> torch.Tensor:
        """(batch, groups + 1) int32 row bounds."""
        return torch.tensor([[self.head + sum(s[:g]) for g in range(len(s) + 1)]
                             for s in self.sizes], dtype=torch.int32)

    @property
    def id(self) -> str:
        grp = (f"{self.groups}x{self.sizes[0][0]}" if self.implicit
               else "b" + "_".join(".".join(map(str, s)) for s in self.sizes) + f"m{self.mgr}")
        return (f"c{self.cols}-x{_name(self.x)}-y{_name(self.out)}-res{_name(self.res)}-"
                f"{'rms' if self.rms else 'ln'}{'-bias' if self.bias else ''}-h{self.head}-{grp}"
                f"{'-rev%d' % self.rev_frame if self.rev_frame else ''}"
                f"{'-sums' if self.sums else ''}")

    def plan_line(self) -> str:
        """The case as ``tests/host/norm_fwd_instance_of.cpp`` reads it (kind 2): batch, rows,
        cols, head, groups, group_rows, max_group_rows, bounds given, x / out dtype codes,
        residual presence and dtype code, rev_frame and the two batch strides of the GPU test's
        padded buffers."""
        return " ".join(str(int(v)) for v in (
            2, POOL_BATCH, self.rows, self.cols, self.head, self.groups,
            self.sizes[0][0] if self.implicit else 0, self.mgr, not self.implicit, _code(self.x),
            _code(self.out), self.res is not None, _code(self.res), self.rev_frame,
            (self.rows + POOL_PAD_ROWS) * self.cols, (self.rows + POOL_OUT_PAD) * self.cols))


def pool_instance(c: PoolCase) -> tuple:
    """("fast", CPL) for ``norm_pool_rows_bf16_kernel``, ("generic", CPL) for
    ``norm_pool_rows_kernel``, as ``vm_norm_pool_fwd`` picks them."""
    cpl = (c.cols + 255) // 256
    if (c.x == BF16 and c.out == BF16 and c.res in (None, F32) and cpl <= 4
            and (c.rows + 1) * c.cols * 4 < 2 ** 31):
        return ("fast", cpl)
    return ("generic", 1 if cpl <= 1 else 2 if cpl <= 2 else 4 if cpl <= 4 else 8)


POOL_INSTANCES = [("fast", c) for c in (1, 2, 3, 4)] + [("generic", c) for c in (1, 2, 4, 8)]

POOL_COLS = (4, 192, 256, 260, 576, 1024, 1028, 2048)
POOL_DTYPES = ((BF16, BF16, None), (BF16, BF16, F32), (BF16, BF16, BF16), (F32, F32, F32),
               (F32, BF16, F32), (BF16, F32, None))                     # (x, out, residual)
POOL_HEADS = (0, 1, 2, 16, 17)
POOL_GROUP_ROWS = (1, 15, 16, 17, 33)
POOL_GROUPS = (1, 3)
# unequal groups, one a single row, max_group_rows above the largest group
POOL_BOUNDS = ((((5, 1, 20), (17, 8, 1)), 33), (((16, 1, 16), (1, 31, 1)), 40))
HEAD_LIMIT = 17  # the largest head in the table: two 16-row slices of head rows


def _frame(rows_after_head: int, groups: int, group_rows: int) -> int:
    """A frame length for ``rev_frame``: the group where there are several, else the smallest
    divisor above 1 (the row count itself when it is prime or 1)."""
    if groups > 1:
        return group_rows
    return next((f for f in range(2, rows_after_head + 1) if rows_after_head % f == 0),
                rows_after_head)


def _pool_cases() -> List[PoolCase]:
    out = []
    shapes = [(g, gr) for gr in POOL_GROUP_ROWS for g in POOL_GROUPS]
    for j, (cols, (xdt, odt, rdt)) in enumerate(itertools.product(POOL_COLS, POOL_DTYPES)):
        rms, bias = NORM_KINDS[(j + j // 6) % 4]
        head = POOL_HEADS[(j + j // 5) % 5]
        k = (j + j // 6) % (len(shapes) + len(POOL_BOUNDS))
        sums = (j + j // 6) % 3 != 0
        if k < len(shapes):
            g, gr = shapes[k]
            rev = _frame(g * gr, g, gr) if head in (0, 1) and (j // 2) % 2 == 0 else 0
            out.append(PoolCase(cols, xdt, odt, rdt, rms, bias, head, ((gr,) * g,) * POOL_BATCH,
                                True, gr, rev, sums))
        else:
            sizes, mgr = POOL_BOUNDS[k - len(shapes)]
            out.append(PoolCase(cols, xdt, odt, rdt, rms, bias, head, sizes, False, mgr, 0, sums))
    # the head rows take more slices than any group (both row kernels, with sums), and a
    # head of exactly one slice
    for xdt, odt, rdt in ((BF16, BF16, F32), (F32, F32, F32)):
        for head, gr in ((17, 1), (16, 15), (17, 33)):
            out.append(PoolCase(260, xdt, odt, rdt, True, False, head, ((gr,) * 3,) * POOL_BATCH,
                                True, gr, 0, True))
    # frames reversed with a head row, in both row kernels, at VideoMamba-M's width
    for xdt, odt, rdt in ((BF16, BF16, F32), (BF16, F32, None)):
        out.append(PoolCase(576, xdt, odt, rdt, True, False, 1, ((17,) * 3,) * POOL_BATCH, True,
                            17, 17, True))
    return out


POOL_CASES = _pool_cases()
# Head rows only: two implicit groups of no rows (max_group_rows 0).  Each group still owns one
# slice of the workspace, which the forward fills with zeros.
HEAD_ONLY = PoolCase(64, BF16, BF16, F32, True, False, 3, ((0, 0),) * POOL_BATCH, True, 0, 0, True)
POOL_PAD_ROWS = 2    # rows of h past `rows` (in_batch_stride padding)
POOL_OUT_PAD = 3     # sentinel rows of out past `rows` in every batch row


def pool_inputs(c: PoolCase, seed: int = 3):
    """Seeded CPU operands: x and residual (batch, rows + POOL_PAD_ROWS, cols) — the padding
    rows hold large values, so a row read from there shows — weight, bias fp32."""
    g = torch.Generator().manual_seed(seed + 11 * c.rows + c.cols)
    shape = (POOL_BATCH, c.rows + POOL_PAD_ROWS, c.cols)
    x = torch.randn(*shape, generator=g)
    x[:, c.rows:] *= 1.0e3
    res = None
    if c.res is not None:
        res = 2.0 * torch.randn(*shape, generator=g)
        res[:, c.rows:] *= 1.0e3
        res = res.to(c.res)
    w = 1.0 + 0.2 * torch.randn(c.cols, generator=g)
    b = 0.2 * torch.randn(c.cols, generator=g) if c.bias else None
    return {"x": x.to(c.x), "residual": res, "weight": w, "bias": b}


def pool_row_map(rows: int, head: int, rev_frame: int) -> torch.Tensor:
    """Input row of every output row: the identity, or with ``rev_frame`` = F > 0 rows
    [head, rows) in reversed frame order, frames of F rows, row order kept within a frame."""
    idx = torch.arange(rows)
    if rev_frame > 0:
        F = rev_frame
        nf = (rows - head) // F
        xr = idx[head:] - head
        idx[head:] = head + (nf - 1 - xr // F) * F + xr % F
    return idx


def norm_pool_ref64(ops, c: PoolCase) -> torch.Tensor:
    """float64 features (batch, rows, cols), not yet rounded."""
    idx = pool_row_map(c.rows, c.head, c.rev_frame)
    x, r = f64(ops["x"])[:, idx], f64(ops["residual"])
    return tbr.add_norm_fwd64(x, None if r is None else r[:, idx], f64(ops["weight"]),
                              f64(ops["bias"]), EPS, c.rms, False)


def slice_sums64(feats: torch.Tensor, bounds: torch.Tensor, slices: int) -> torch.Tensor:
    """float64 column sums of ``feats`` (batch, >= rows, cols) as stored, per (batch row,
    group, POOL_RB-row slice): (batch, groups, slices, cols), zeros past a group's end."""
    ft = f64(feats)
    Bz, G = bounds.shape[0], bounds.shape[1] - 1
    out = torch.zeros(Bz, G, slices, ft.shape[-1], dtype=F64)
    for b in range(Bz):
        for g in range(G):
            lo, hi = int(bounds[b, g]), int(bounds[b, g + 1])
            for s in range(slices):
                out[b, g, s] = ft[b, min(hi, lo + s * POOL_RB):min(hi, lo + (s + 1) * POOL_RB)].sum(0)
    return out


def live_slices(bounds: torch.Tensor, slices: int) -> torch.Tensor:
    """(batch, groups, slices) bool: the slice holds at least one row of its group."""
    n = (bounds[:, 1:] - bounds[:, :-1]).long()
    return torch.arange(slices)[None, None, :] * POOL_RB < n[:, :, None]


# --------------------------------------------------------------------------- pool finish
POOL_MODES = ("avg", "cls+avg", "cls_cat_avg", "cls")


class FinishCase(NamedTuple):
    """One ``vm_pool_finish_fwd`` call on a workspace the test writes.  ``counts``: the group
    row counts of each batch row (passed as ``bounds`` unless ``implicit``); ``cls``: the dtype
    of the CLS rows (their batch stride is larger than cols)."""
    cols: int
    slices: int
    mode: str
    keep_temporal: bool
    counts: Tuple[Tuple[int, ...], ...]
    implicit: bool
    xp: torch.dtype
    cls: torch.dtype
    lnw: bool
    lnb: bool

    @property
    def groups(self) -> int:
        return len(self.counts[0])

    @property
    def mgr(self) -> int:
        return self.slices * POOL_RB

    @property
    def prow(self) -> int:
        navg = self.groups if self.keep_temporal else 1
        return {"cls": 1, "cls_cat_avg": 1 + navg}.get(self.mode, navg)

    def bounds(self) -> torch.Tensor:
        return torch.tensor([[1 + sum(s[:g]) for g in range(len(s) + 1)] for s in self.counts],
                            dtype=torch.int32)

    @property
    def id(self) -> str:
        return (f"c{self.cols}-s{self.slices}-{self.mode}{'-keep' if self.keep_temporal else ''}-"
                f"{'impl' if self.implicit else 'bounds'}{self.groups}-xp{_name(self.xp)}-"
                f"cls{_name(self.cls)}{'-w' if self.lnw else ''}{'-b' if self.lnb else ''}")


FINISH_COLS = (4, 576, 1024, 1028, 2048)
FINISH_SLICES = (1, 5, 13)


def _finish_cases() -> List[FinishCase]:
    out = []
    for j, (cols, slices, mode) in enumerate(itertools.product(FINISH_COLS, FINISH_SLICES,
                                                               POOL_MODES)):
        top = slices * POOL_RB
        implicit = (j + j // 4) % 2 == 0
        if implicit:   # the last slice of every group one row short of full
            counts = ((top - 1,) * 3,) * POOL_BATCH
        else:          # short groups: their last slices are zeros
            counts = ((top, 1, max(1, top // 2)), (max(1, top - 17), top, 2))
        xp = (F32, BF16)[(j // 4 + j // 2) % 2]
        out.append(FinishCase(cols, slices, mode, (j + j // 8) % 2 == 0, counts, implicit, xp,
                              xp if j % 5 else _other(xp), (j // 3) % 2 == 0, (j // 3) % 4 < 2))
    return out


FINISH_CASES = _finish_cases()


def finish_inputs(c: FinishCase, seed: int = 5):
    """Seeded CPU operands: the workspace (batch, groups, slices, cols) fp32 of multiples of
    2^-6 in [-4, 4] — every fp32 summation order of them is exact — the CLS rows (batch, cols)
    in ``c.cls``, LayerNorm weight and bias fp32 or None."""
    g = torch.Generator().manual_seed(seed + c.cols + 13 * c.slices)
    ws = torch.randint(-256, 257, (POOL_BATCH, c.groups, c.slices, c.cols), generator=g).float() / 64
    cls = torch.randn(POOL_BATCH, c.cols, generator=g).to(c.cls)
    w = 1.0 + 0.2 * torch.randn(c.cols, generator=g) if c.lnw else None
    b = 0.2 * torch.randn(c.cols, generator=g) if c.lnb else None
    return {"ws": ws, "cls": cls, "lnw": w, "lnb": b}


def pool_finish_ref64(ws, counts, cls, mode: str, keep_temporal: bool, lnw, lnb, ln_eps: float,
                      xp: torch.dtype) -> torch.Tensor:
    """float64 x_pool (batch, P, cols).  ws: (batch, groups, slices, cols) slice sums; counts:
    (batch, groups) rows per group; cls: (batch, cols) or None."""
    sums = f64(ws).sum(2)
    cnt = f64(torch.as_tensor(counts))
    if keep_temporal:
        avg = sums / cnt[:, :, None]
    else:
        avg = sums.sum(1, keepdim=True) / cnt.sum(1)[:, None, None]
    avg = avg.to(xp).to(F64)
    c = None if cls is None else f64(cls)[:, None]
    if mode == "cls":
        v = c
    elif mode == "avg":
        v = avg
    elif mode == "cls+avg":
        v = (c + avg).to(xp).to(F64)
    else:
        v = torch.cat([c, avg], 1)
    return layer_norm_ref64(v, f64(lnw), f64(lnb), ln_eps)


# --------------------------------------------------------------------------- one-token steps
STEP_DTYPES = ((F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16))   # (x, state)
STEP_BATCH, STEP_DIM, STEP_N, STEP_W = (1, 3), (1, 24, 257), (1, 16, 17), (1, 2, 4, 5, 8)
SOFTPLUS_THRESHOLD = 20.0


class StepCase(NamedTuple):
    batch: int
    dim: int
    n: int
    x: torch.dtype
    state: torch.dtype
    D: bool
    z: bool
    dt_bias: bool
    softplus: bool

    @property
    def id(self) -> str:
        on = [k for k in ("D", "z", "dt_bias", "softplus") if getattr(self, k)]
        return (f"b{self.batch}-d{self.dim}-n{self.n}-x{_name(self.x)}-s{_name(self.state)}-"
                + "+".join(on or ["bare"]))


class ConvStepCase(NamedTuple):
    batch: int
    dim: int
    width: int
    x: torch.dtype
    state: torch.dtype
    bias: bool
    silu: bool

    @property
    def id(self) -> str:
        return (f"b{self.batch}-d{self.dim}-w{self.width}-x{_name(self.x)}-s{_name(self.state)}"
                f"{'-bias' if self.bias else ''}{'-silu' if self.silu else ''}")


def _step_cases():
    out = []
    for j, (b, d, n) in enumerate(itertools.product(STEP_BATCH, STEP_DIM, STEP_N)):
        xdt, sdt = STEP_DTYPES[j % 4]
        out.append(StepCase(b, d, n, xdt, sdt, j % 3 != 0, j % 3 != 1, j % 3 != 2,
                            (j // 4) % 2 == 1))
    return out


def _conv_step_cases():
    out = []
    for j, (b, d, w) in enumerate(itertools.product(STEP_BATCH, STEP_DIM, STEP_W)):
        xdt, sdt = STEP_DTYPES[(j + j // 4) % 4]
        out.append(ConvStepCase(b, d, w, xdt, sdt, (j // 2) % 2 == 0, (j + j // 5 + j // 10) % 2 == 0))
    return out


STEP_CASES, CONV_STEP_CASES = _step_cases(), _conv_step_cases()


def step_inputs(c: StepCase, seed: int = 9):
    """Seeded CPU operands of the SSM step.  Without softplus the raw step is positive,
    ``dt = 0.05 + 0.3 |randn|``.  With it ``dt = 2 randn`` and on every third channel
    ``dt + dt_bias`` is spread over [17, 24], both sides of softplus's large-argument branch at
    20; those channels' x is scaled by 1/20 so the outputs stay of one size."""
    g = torch.Generator().manual_seed(seed + c.dim + 3 * c.n)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    state, x, noise = rn(c.batch, c.dim, c.n), rn(c.batch, c.dim), rn(c.batch, c.dim)
    A = -torch.exp(torch.log(torch.arange(1, c.n + 1).float()).repeat(c.dim, 1) + 0.1 * rn(c.dim, c.n))
    Bm, Cm, Dv, z = rn(c.batch, c.n), rn(c.batch, c.n), rn(c.dim), rn(c.batch, c.dim)
    rnd = torch.rand(c.batch, c.dim, generator=g)
    if c.softplus:
        bias = 0.5 * rn(c.dim)
        dt = 2.0 * noise
        big = torch.arange(c.dim) % 3 == 0
        target = 17.0 + 7.0 * rnd
        dt[:, big] = (target - (bias[None] if c.dt_bias else 0.0))[:, big]
        x[:, big] *= 0.05
    else:
        bias = 0.1 * torch.rand(c.dim, generator=g)
        dt = 0.05 + 0.3 * noise.abs()
    return {"state": state.to(c.state), "x": x.to(c.x), "dt": dt.to(c.x), "A": A,
            "B": Bm.to(c.x), "C": Cm.to(c.x), "D": Dv if c.D else None,
            "z": z.to(c.x) if c.z else None, "dt_bias": bias if c.dt_bias else None}


def conv_step_inputs(c: ConvStepCase, seed: int = 13):
    g = torch.Generator().manual_seed(seed + c.dim + 5 * c.width)
    return {"x": torch.randn(c.batch, c.dim, generator=g).to(c.x),
            "conv_state": torch.randn(c.batch, c.dim, c.width, generator=g).to(c.state),
            "weight": 0.5 * torch.randn(c.dim, c.width, generator=g),
            "bias": 0.5 * torch.randn(c.dim, generator=g) if c.bias else None}


def softplus64(v: torch.Tensor) -> torch.Tensor:
    """torch's softplus (beta 1, threshold 20) in float64."""
    return torch.where(v > SOFTPLUS_THRESHOLD, v,
                       torch.log1p(torch.exp(torch.clamp(v, max=SOFTPLUS_THRESHOLD))))


def ssm_step_ref64(state, x, dt, A, B, C, D=None, z=None, dt_bias=None, softplus=False):
    """float64 one-token scan step: (out (b, d), new state (b, d, n)), neither rounded.  The
    state is read as stored; the output uses the new state before its store rounds it."""
    state, x, dt, A, B, C, D, z, dt_bias = map(f64, (state, x, dt, A, B, C, D, z, dt_bias))
    if dt_bias is not None:
        dt = dt + dt_bias[None]
    if softplus:
        dt = softplus64(dt)
    new = state * torch.exp(dt[..., None] * A[None]) + (dt * x)[..., None] * B[:, None, :]
    out = (new * C[:, None, :]).sum(-1)
    if D is not None:
        out = out + x * D[None]
    if z is not None:
        out = out * (z / (1.0 + torch.exp(-z)))
    return out, new


def conv_step_ref64(x, conv_state, weight, bias, silu: bool):
    """One-token conv step: (out (b, d) float64, the new state in ``conv_state``'s dtype).  The
    state shifts left by one and takes x, rounded once to the state's dtype; the dot runs over
    the state as stored."""
    new = torch.cat([conv_state[..., 1:], x[..., None].to(conv_state.dtype)], -1)
    out = (f64(new) * f64(weight)[None]).sum(-1)
    if bias is not None:
        out = out + f64(bias)[None]
    if silu:
        out = out / (1.0 + torch.exp(-out))
    return out, new
