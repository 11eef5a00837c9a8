"""Every kernel form of the selective scan against the float64 reference of
``scan_matrix.py``, over the option table (D / z / bias / softplus / state handling).

``vm_selective_scan_fwd`` dispatches on layout, dtype, grid size, segment count, B/C layout
and the optional operands; each test below names the form it reaches and the dispatch
condition it relies on, asserts what the ABI lets it probe (``scan_chunk_steps``, the sync
buffer's size and header), then compares ``y`` — for bf16 operands with the reference
rounded once to bf16 — and, where the row has one, ``h_last``.  Tolerances are those of
``test_gpu_parity.py``: fp32 y 1e-4, bf16 y 2e-2, fp32 state 1e-4, bf16-stored state 1e-2
(abs+rel).  The fp32 oracle sits ~5e-7 from the reference, so 1e-4 leaves two orders of
magnitude for exp2 / FMA-order differences.

Largest observed |got - ref| / (tol + tol |ref|) per form and dtype on an MI355X (the share
of each tolerance in use; printed again by every run with ``-s``):

    form                   fp32 y  fp32 h_last  bf16 y  bf16 h_last
    cm-bf16-pipe              -            -     0.105        0.150
    cm-bf16-pipe-D12          -            -     0.188        0.113
    cm-bf16-plain-k10         -            -     0.340        0.253
    cm-bf16-plain-k8          -            -     0.222        0.255
    cm-bf16-plain-k8-L600     -            -     0.305        0.254
    cm-bf16-split             -            -     0.160        0.164
    cm-fp32-k10             0.334        0.155     -            -
    cm-fp32-k8              0.116        0.137     -            -
    cm-fp32-k8-L600         0.153        0.159     -            -
    pair-chunk1             0.093        0.251   0.222        0.252
    pair-chunk1-carry       0.076        0.027   0.113        0.035
    pair-chunk2             0.093        0.251   0.222        0.252
    pair-chunk2-carry       0.076        0.027   0.113        0.035
    pair-single             0.091        0.251   0.243        0.252
    tm-chunk1-bc1           0.075        0.248   0.207        0.240
    tm-chunk1-bc1-carry     0.076        0.027   0.000        0.035
    tm-chunk1-sep           0.075        0.248   0.207        0.240
    tm-chunk1-sep-carry     0.076        0.027   0.000        0.035
    tm-chunk2-bc1           0.075        0.248   0.207        0.240
    tm-chunk2-bc1-carry     0.076        0.027   0.000        0.035
    tm-chunk2-sep           0.075        0.248   0.207        0.240
    tm-chunk2-sep-carry     0.076        0.027   0.000        0.035
    tm-legacy               0.070        0.178   0.281        0.188
    tm-legacy-carry         0.043        0.015   0.006        0.023
    tm-single-bc1           0.080        0.248   0.243        0.240
    tm-single-sep           0.080        0.248   0.243        0.240
    tm-single-vec           0.075        0.178   0.281        0.188

(h_last of a form takes the row's tolerance: 1e-2 for the bf16 state updated in place, 1e-4
otherwise; "-carry" is the L = 24 one-step-per-segment case; 0.000 = every element equal to
the rounded reference.)
"""

import ctypes

import pytest
import torch

import scan_matrix as sm
from videomamba_amd import _lib
from videomamba_amd import kernels as K
from videomamba_amd import options

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
SENTINEL = 7.0
R_PAD = 8  # x_dbl columns before B | C in the mixer layout (the dt_low slot)

_dtid = lambda dt: "bf16" if dt == BF16 else "fp32"  # noqa: E731
_rowid = lambda r: r.id  # noqa: E731

_CASES = {}   # (row, dtype, shape, pair) -> inputs, computed once
_REFS = {}    # ... + frame -> float64 reference, computed once and never modified
RATIOS = {}   # (form, dtype id) -> [worst y ratio, worst h_last ratio]


@pytest.fixture(autouse=True, scope="module")
def _gpu_and_report():
    assert torch.cuda.is_available(), "gpu-marked tests need a HIP device"
    yield
    print("\nscan matrix: largest |got - ref| / (tol + tol |ref|)   form  dtype  y  h_last")
    for (form, dt), (ry, rh) in sorted(RATIOS.items()):
        print(f"  {form:<22} {dt:<5} {ry:6.3f} {rh:6.3f}")


def _inputs(row, dt, shape):
    key = (row, dt, shape)
    if key not in _CASES:
        _CASES[key] = sm.make_inputs(row, dt, *shape, seed=1)
        _REFS[key] = _CASES[key].ref(row.softplus)
    return _CASES[key], _REFS[key]


def _pair_inputs(row, dt, split, shape, frame):
    key = (row, dt, shape, "pair")
    if key not in _CASES:
        _CASES[key] = sm.make_pair_inputs(row, dt, split, *shape, seed=1)
    if key + (frame,) not in _REFS:
        _REFS[key + (frame,)] = _CASES[key].ref(row.softplus, frame)
    return _CASES[key], _REFS[key + (frame,)]


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _tm(t):
    """Same (b, d, l) values stored token-major (unit channel stride)."""
    return None if t is None else t.transpose(1, 2).contiguous().transpose(1, 2)


def _record(form, dt, ry, rh):
    cur = RATIOS.setdefault((form, _dtid(dt)), [0.0, 0.0])
    cur[0], cur[1] = max(cur[0], ry), max(cur[1], rh)


class _State:
    """Device state tensors of a row: h0, h_last (the same tensor for the in-place bf16
    state), and a sentinel-filled tensor that is never passed to the kernel."""

    def __init__(self, row, h0_cpu, Bz, D, N):
        self.row = row
        self.h0 = _dev(h0_cpu)
        self.h0_before = None if self.h0 is None else self.h0.clone()
        self.guard = torch.full((Bz, D, N), SENTINEL, device=DEV)
        if row.state == "bf16_inplace":
            self.hl = self.h0
        elif row.has_hl:
            self.hl = torch.full((Bz, D, N), SENTINEL, device=DEV)
        else:
            self.hl = None

    def strides(self, t):
        return (0, 0) if t is None else (t.stride(0), t.stride(1))

    def check(self, ref_h, what):
        """h_last against the reference; an h0 that is not also h_last, and the tensor
        that was never passed, come back untouched."""
        assert torch.equal(self.guard, torch.full_like(self.guard, SENTINEL)), what
        if self.h0 is not None and self.hl is not self.h0:
            assert torch.equal(self.h0, self.h0_before), f"{what}: h0 was written"
        if self.hl is None:
            return 0.0
        return sm.assert_within(self.hl, ref_h, self.row.state_tol, f"{what} h_last")


def _check_y(y, ref_y, dt, what):
    return sm.assert_within(y.float(), sm.round_like(ref_y, dt).float(), sm.TOL_Y[dt],
                            f"{what} y")


def _via_selective_scan_fn(row, dt, inp, ref, tm, what, st=None):
    """The mamba-ssm drop-in on channel-major (``tm`` False) or token-major views."""
    Bz, D, L = inp.u.shape
    N = inp.A.shape[1]
    st = st or _State(row, inp.h0, Bz, D, N)
    lay = (lambda t: _tm(_dev(t))) if tm else _dev
    res = K.selective_scan_fn(lay(inp.u), lay(inp.delta), _dev(inp.A), lay(inp.B), lay(inp.C),
                              D=_dev(inp.D), z=lay(inp.z), delta_bias=_dev(inp.bias),
                              delta_softplus=row.softplus, return_last_state=row.has_hl,
                              initial_state=st.h0, last_state_out=st.hl)
    y = res[0] if row.has_hl else res
    assert y.dtype == dt and y.shape == (Bz, D, L)
    assert (y.stride(1) == 1) == tm
    if row.has_hl:
        assert res[1] is st.hl
    ry = _check_y(y, ref[0], dt, what)
    rh = st.check(ref[1], what)
    return ry, rh


class _MixerLayout:
    """The token-major mixer's operand layout (mamba_simple._forward_padded_tm): u / delta /
    y rows (B Lp, D) with Lp = round_up(L, 8) and zero padding rows, z the second half of
    the xz rows, B and C adjacent columns of one x_dbl row (C directly after B: the BC1
    form).  y is pre-filled with a sentinel: rows >= L must come back zero."""

    def __init__(self, inp, dt):
        Bz, D, L = inp.u.shape
        N = inp.A.shape[1]
        E = R_PAD + 2 * N
        Lp = (L + 7) // 8 * 8
        rows = lambda t: t.transpose(1, 2)  # noqa: E731  (b, d, l) -> (b, l, d)
        U = torch.zeros(Bz, Lp, D, dtype=dt)
        DL = torch.zeros(Bz, Lp, D, dtype=dt)
        XD = torch.zeros(Bz, Lp, E, dtype=dt)
        U[:, :L], DL[:, :L] = rows(inp.u), rows(inp.delta)
        XD[:, :L, R_PAD:R_PAD + N], XD[:, :L, R_PAD + N:] = rows(inp.B), rows(inp.C)
        self.U, self.DL, self.XD = (t.reshape(Bz * Lp, -1).to(DEV) for t in (U, DL, XD))
        self.Zv, self.s_z = None, (0, 0, 0)
        if inp.z is not None:
            XZ = torch.zeros(Bz, Lp, 2 * D, dtype=dt)
            XZ[:, :L, D:] = rows(inp.z)
            self.XZ = XZ.reshape(Bz * Lp, -1).to(DEV)
            self.Zv, self.s_z = self.XZ[:, D:], (Lp * 2 * D, 1, 2 * D)
        self.Bv, self.Cv = self.XD[:, R_PAD:R_PAD + N], self.XD[:, R_PAD + N:]
        self.s_u, self.s_bc = (Lp * D, 1, D), (Lp * E, 1, E)
        self.y = torch.full((Bz * Lp, D), SENTINEL, dtype=dt, device=DEV)
        self.dims = (Bz, D, L, N, Lp)

    def run(self, inp, row, dt, st, pair=None):
        Bz, D, L, N, Lp = self.dims
        K.scan_raw(self.U, self.s_u, self.DL, self.s_u, _dev(inp.A), self.Bv, self.s_bc,
                   self.Cv, self.s_bc, _dev(inp.D), self.Zv, self.s_z, _dev(inp.bias),
                   row.softplus, st.h0, st.strides(st.h0), st.hl, st.strides(st.hl), self.y,
                   self.s_u, Lp, Bz, D, L, N, K.dtype_code(dt),
                   torch.cuda.current_stream().cuda_stream, pair=pair)
        y = self.y.view(Bz, Lp, D)
        assert not y[:, L:].float().abs().any(), "padding rows must come back zero"
        return y[:, :L].transpose(1, 2)


def _via_mixer_layout(row, dt, inp, ref, what):
    Bz, D, L = inp.u.shape
    st = _State(row, inp.h0, Bz, D, inp.A.shape[1])
    y = _MixerLayout(inp, dt).run(inp, row, dt, st)
    return _check_y(y, ref[0], dt, what), st.check(ref[1], what)


class _sync_probe:
    """A zeroed sync buffer of the shape's size for a one-launch case; after the launch its
    header must read [no error, epoch 1, start count 0] (ABI v9) — which also shows the
    one-launch form ran: the two-launch form never touches the buffer."""

    def __init__(self, one_launch, Bz, D, L, N, segments):
        self.on = one_launch
        if one_launch:
            nbytes = K.scan_sync_bytes(Bz, D, L, N, segments)
            assert nbytes > 0
            self.buf = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
            self.ctx = K.sync_override(self.buf)

    def __enter__(self):
        if self.on:
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.on:
            self.ctx.__exit__(*exc)
            if exc[0] is None:
                head = self.buf[:16].view(torch.int32).cpu().tolist()
                assert head[:3] == [0, 1, 0], head
        return False


# ------------------------------------------------------------------- token-major forms
# form -> (dstate, B/C layout, scan_segments, scan_one_launch, steps per segment)
TM_FORMS = {
    "tm-single-sep": (16, "sep", 1, True, 0),
    "tm-single-bc1": (16, "bc1", 1, True, 0),
    "tm-single-vec": (8, "sep", 1, True, 0),
    "tm-legacy": (8, "sep", 7, True, 22),
    "tm-chunk2-sep": (16, "sep", 20, False, 8),
    "tm-chunk2-bc1": (16, "bc1", 20, False, 8),
    "tm-chunk1-sep": (16, "sep", 20, True, 8),
    "tm-chunk1-bc1": (16, "bc1", 20, True, 8),
}


def _run_tm_form(form, row, dt, L, steps=None):
    N, layout, segments, one, T = TM_FORMS[form]
    T = T if steps is None else steps
    segments = segments if steps is None else L
    Bz, D = 2, 136
    assert K.scan_chunk_steps(Bz, D, L, N, segments) == T
    inp, ref = _inputs(row, dt, (Bz, D, L, N))
    what = f"{form} {row.id} {_dtid(dt)} L={L}"
    chunked = T > 0 and N == 16
    with options.override(scan_segments=segments, scan_one_launch=one), \
            _sync_probe(one and chunked, Bz, D, L, N, segments):
        if layout == "sep":
            ry, rh = _via_selective_scan_fn(row, dt, inp, ref, True, what)
        else:
            ry, rh = _via_mixer_layout(row, dt, inp, ref, what)
    _record(form if steps is None else form + "-carry", dt, ry, rh)


@pytest.mark.parametrize("row", sm.ROWS, ids=_rowid)
@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
@pytest.mark.parametrize("form", sorted(TM_FORMS))
def test_token_major_form_matches_ref64(form, dt, row):
    """(2, 136, 150, N): D = 136 is two full 64-channel waves and one with 8 live lanes —
    and in scan_seq_kernel a wholly dead fourth wave (the d0 clamp, kSeqDead stores).
    Dispatch relied on (vm_scan_plan.h::plan_scan, then vm_scan_seq.hip seq_launch -> launch_seq / launch_chunk):
    * single: ``scan_segments=1`` -> scan_seq_kernel MODE 0; scalar-load B/C when
      seq_sgpr_bc holds (N = 16, unit state stride, 4-byte aligned rows: the ``_tm`` views
      and the mixer layout), BC1 when C directly follows B in one row (mixer layout only),
      the LDS-staged vector B/C kernel at N = 8;
    * legacy: N = 8 with ``scan_segments=7`` -> MODE 1, scan_seq_carry_kernel, MODE 2 over
      22-step segments (the last one ragged: 18 steps);
    * chunk2 / chunk1: N = 16 with ``scan_segments=20`` -> scan_chunk_kernel with T = 8, 19
      segments, 3 blocks of kChW = 8 (the last with 3 live waves, the last segment 6 steps);
      PASS 1 + PASS 2 with ``scan_one_launch=False``, PASS 3 with the sync buffer otherwise
      (grid 3 x 3 x 2 = 18 workgroups, resident on any part).
    "sep" cases go through selective_scan_fn on ``_tm`` views, "bc1" through K.scan_raw on
    the mixer layout with out_len = Lp = 152 (padding rows must come back zero)."""
    _run_tm_form(form, row, dt, 150)


CARRY_ROW = sm.ROWS[1]  # everything present, fp32 h0 and a separate fp32 h_last
assert CARRY_ROW == sm.Row(True, True, True, True, "h0_hl")


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
@pytest.mark.parametrize("form", [f for f in sorted(TM_FORMS) if TM_FORMS[f][4] > 0])
def test_segmented_form_carries_h0_through_every_segment(form, dt):
    """L = 24 with ``scan_segments=24``: one step per segment, three blocks of eight, so
    every element of h_last depends on h0 through the whole carry chain (the segment
    carries and, in the chunked forms, the block aggregates).  At this shape u / delta / z
    (2 x 24 x 136) and the separate B (2 x 24 x 16) fill whole 512-byte allocator blocks,
    so a read past an operand's end leaves its allocation: the fp32 one-launch case met an
    illegal memory access once, from scan_chunk_kernel's lanes past dim loading at
    lane * ES and its separate-B warm-up span of two rows (both fixed with this test)."""
    _run_tm_form(form, CARRY_ROW, dt, 24, steps=1)


# ------------------------------------------------------------------- paired forms
PAIR_FORMS = {"pair-single": (1, True, 0), "pair-chunk2": (20, False, 8),
              "pair-chunk1": (20, True, 8)}


def _run_pair_form(form, row, dt, L, frame, steps=None):
    segments, one, T = PAIR_FORMS[form]
    T = T if steps is None else steps
    segments = segments if steps is None else L
    split, D, N = 2, 136, 16
    Bz = 2 * split
    assert K.scan_chunk_steps(Bz, D, L, N, segments) == T
    pi, (ref_y, ref_hf, ref_hb) = _pair_inputs(row, dt, split, (D, L, N), frame)
    what = f"{form} F={frame} {row.id} {_dtid(dt)} L={L}"
    st_f = _State(row, pi.both.h0, split, D, N)
    st_b = _State(row, pi.h0_b, split, D, N)
    lay = _MixerLayout(pi.both, dt)
    pair = (split, _dev(pi.A_b), _dev(pi.D_b), _dev(pi.bias_b), st_b.h0, st_b.hl, frame)
    with options.override(scan_segments=segments, scan_one_launch=one), \
            _sync_probe(one and T > 0, Bz, D, L, N, segments):
        y = lay.run(pi.both, row, dt, st_f, pair=pair)
    ry = _check_y(y, ref_y, dt, what)
    rh = max(st_f.check(ref_hf, what + " fwd"), st_b.check(ref_hb, what + " bwd"))
    _record(form if steps is None else form + "-carry", dt, ry, rh)


@pytest.mark.parametrize("row", sm.ROWS, ids=_rowid)
@pytest.mark.parametrize("frame", [1, 25])
@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
@pytest.mark.parametrize("form", sorted(PAIR_FORMS))
def test_paired_form_matches_ref64(form, dt, frame, row):
    """vm_selective_scan_bidir_fwd over 2 + 2 rows of (136, 150, 16) in the mixer layout:
    rows >= split scan with their own A / D / bias / h0 (a row without D / bias / h0 drops
    it for both directions) and store step t at row t + (L - F) - 2F floor(t / F) (L - 1 - t
    for F = 1).  ``p.split < p.batch`` selects the PAIR instantiations: of scan_seq_kernel
    with ``scan_segments=1`` (launch_seq), of scan_chunk_kernel with
    ``scan_segments=20`` (launch_chunk), two launches or one as above (grid 3 x 3 x 4)."""
    _run_pair_form(form, row, dt, 150, frame)


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
@pytest.mark.parametrize("form", ["pair-chunk1", "pair-chunk2"])
def test_paired_chunked_form_carries_h0_through_every_segment(form, dt):
    """The L = 24, one-step-per-segment carry case on the paired chunked forms."""
    _run_pair_form(form, CARRY_ROW, dt, 24, 1, steps=1)


# ------------------------------------------------------------------- channel-major forms
CM_FORMS = {
    "cm-fp32-k8": (F32, (2, 24, 300, 16)),
    "cm-fp32-k8-L600": (F32, (2, 24, 600, 16)),
    "cm-fp32-k10": (F32, (2, 24, 1300, 16)),
    "cm-bf16-split": (BF16, (1, 12, 1300, 16)),
    "cm-bf16-pipe": (BF16, (2, 24, 300, 16)),
    "cm-bf16-pipe-D12": (BF16, (1, 12, 600, 16)),
    "cm-bf16-plain-k8": (BF16, (30, 72, 100, 16)),
    "cm-bf16-plain-k8-L600": (BF16, (30, 72, 600, 16)),
    "cm-bf16-plain-k10": (BF16, (30, 72, 1300, 16)),
}


@pytest.mark.parametrize("row", sm.ROWS, ids=_rowid)
@pytest.mark.parametrize("form", sorted(CM_FORMS))
def test_channel_major_form_matches_ref64(form, row):
    """Step-contiguous operands take scan_v5_kernel; launch_v5_auto (vm_scan.hip) picks the
    steps per lane: K = 10 when cost(10) <= cost(8), else 8.  ``cost(k)`` is written as
    ``((out_len + 64k - 1) / 64k) * 64k * (1 + 4/k)`` in double arithmetic, with no
    rounding down to whole blocks, so it is (L + 64k - 1)(1 + 4/k) and K = 10 holds exactly
    for L >= 1281 — not for the L in (512, 640] that whole 640-step blocks would favour.
    L = 1300 (two 640-step blocks and a ragged 20) reaches K = 10; L = 100, 300 and 600 run
    K = 8.  For bf16 only: the state-split form launch_v5_split<10, 10, 2> when
    ceil(dim / 8) batch <= 256 and K = 10 ((1, 12, 1300): 5 channels per workgroup, ragged),
    the pipelined form PIPE=true when the grid ceil(dim / 8) x batch <= 256 and K = 8
    ((2, 24, 300): 6 workgroups; (1, 12, 600): ragged 8-channel groups), the plain form
    above that ((30, 72, L): 270 workgroups).  fp32 runs the plain form only."""
    dt, shape = CM_FORMS[form]
    inp, ref = _inputs(row, dt, shape)
    ry, rh = _via_selective_scan_fn(row, dt, inp, ref, False, f"{form} {row.id}")
    _record(form, dt, ry, rh)


# ------------------------------------------------------------------- rejection
@pytest.mark.parametrize("case", ["z-null", "softplus-off", "softplus-off-segmented"])
def test_dtproj_entry_rejects_missing_z_and_softplus_off(case):
    """vm_selective_scan_dtproj_fwd exists for z present and softplus on only.  Both are
    checked on the host before any launch (``!z`` at the top of the entry; ``p.softplus``
    in seq_dtp_supported for the single pass and in seq_dtp_chunk_supported for the
    segmented form), so the call returns VM_E_INVALID, vm_last_error names the entry, and
    the output buffer keeps its sentinel."""
    lib = _lib.load()
    Bz, D, L, N, R = 1, 128, 40, 16, 12
    E, Lp = R + 2 * N, 40
    segments = 5 if case.endswith("segmented") else 1
    assert (K.scan_chunk_steps(Bz, D, L, N, segments) > 0) == (segments > 1)
    g = torch.Generator().manual_seed(3)
    mk = lambda *s: torch.randn(*s, generator=g).to(BF16).to(DEV)  # noqa: E731
    U, XZ, XD = mk(Bz * Lp, D), mk(Bz * Lp, 2 * D), mk(Bz * Lp, E)
    wdt = torch.zeros(D, 32, dtype=BF16, device=DEV)
    A = -torch.rand(D, N, generator=g).to(DEV)
    y = torch.full((Bz * Lp, D), SENTINEL, dtype=BF16, device=DEV)
    ws_bytes = K.scan_workspace_bytes(Bz, D, L, N, segments)
    ws = torch.zeros(max(ws_bytes, 16), dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    s_u, s_z, s_bc = (Lp * D, 1, D), (Lp * 2 * D, 1, 2 * D), (Lp * E, 1, E)
    def call(z, softplus):
        return lib.vm_selective_scan_dtproj_fwd(
            p(U), *s_u, p(XD), Lp * E, E, R, p(wdt), 32, p(A),
            p(XD[:, R:R + N]), *s_bc, p(XD[:, R + N:]), *s_bc, None, z, *s_z, None, softplus,
            None, 0, 0, 0, None, 0, 0, 0, p(y), *s_u, Lp, Bz, D, L, N, _lib.VM_DTYPE_BF16,
            segments, p(ws), ws_bytes, None, 0, torch.cuda.current_stream().cuda_stream)

    bad_z = None if case == "z-null" else p(XZ[:, D:])
    rc = call(bad_z, 0 if case.startswith("softplus-off") else 1)
    assert rc == -1  # VM_E_INVALID
    assert b"vm_selective_scan_dtproj_fwd" in lib.vm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full_like(y, SENTINEL))
    # the same call with z and softplus on is accepted: nothing else was wrong with it
    assert call(p(XZ[:, D:]), 1) == 0
    torch.cuda.synchronize()
    assert not (y.float() == SENTINEL).all()
