"""Keeps the scan option matrix honest without a GPU: the float64 reference against the
recorded fixtures, the paired reference against explicit flips, the option table's covering
properties, and the inputs' sensitivity — every operand a row has must matter to the
outputs by far more than the tolerance the GPU tests compare with."""

import pytest
import torch

import scan_matrix as sm
from conftest import load_golden

SCAN, SCAN_META = load_golden("scan_cases.npz")
DTYPES = [torch.float32, torch.bfloat16]
_dtid = lambda dt: "bf16" if dt == torch.bfloat16 else "fp32"  # noqa: E731


@pytest.mark.parametrize("name", sorted(SCAN_META))
def test_ref64_matches_reference_fixture(name):
    """Tolerances of test_oracle_golden.py: 2e-5 for fp32 cases and every last state; bf16
    outputs within one bf16 rounding (2e-2 abs+rel)."""
    meta = SCAN_META[name]
    dt = torch.bfloat16 if meta["dtype"] == "bfloat16" else torch.float32
    g = lambda k, d=dt: torch.from_numpy(SCAN[f"{name}/{k}"].copy()).to(d)  # noqa: E731
    opt = lambda k, d=dt: g(k, d) if f"{name}/{k}" in SCAN.files else None  # noqa: E731
    y, h = sm.scan_ref64(g("u"), g("delta"), g("A", torch.float32), g("B"), g("C"),
                         opt("D", torch.float32), opt("z"), opt("delta_bias", torch.float32),
                         meta["softplus"], opt("initial_state", torch.float32))
    sm.assert_within(g("out", torch.float32), y, 2e-5 if dt == torch.float32 else 2e-2, "out")
    sm.assert_within(g("last_state", torch.float32), h, 2e-5, "last_state")


def _frame_flip(t, F):
    """Explicit reversal of the frame order along the last axis (frames of F steps)."""
    *lead, L = t.shape
    return torch.flip(t.reshape(*lead, L // F, F), dims=[-2]).reshape(*lead, L)


@pytest.mark.parametrize("F", [1, 5, 30])
def test_ref64_paired_equals_explicit_flips(F):
    """The backward half of a bidirectional block scans the frame-flipped sequence and its
    output is flipped back (refiner_backbone.BiMambaRefinerBlock): scan_ref64_paired on the
    flipped operands must equal scan_ref64 on them with the output flipped explicitly, for
    F = 1 (plain reversal), an inner frame size and F = L (identity), each direction with
    its own A / D / bias / h0; the forward half is the plain scan."""
    row = sm.Row(True, True, True, True, "h0_hl")
    L, split = 30, 2
    pi = sm.make_pair_inputs(row, torch.float32, split, 9, L, 16, 5)
    i = pi.both
    flip3 = lambda t: torch.cat([t[:split], _frame_flip(t[split:], F)], 0)  # noqa: E731
    # ``i`` holds the un-flipped sequence in its second half; the entry takes it flipped
    y, h_f, h_b = sm.scan_ref64_paired(flip3(i.u), flip3(i.delta), i.A, flip3(i.B), flip3(i.C),
                                       i.D, flip3(i.z), i.bias, True, i.h0, split, pi.A_b,
                                       pi.D_b, pi.bias_b, pi.h0_b, F)
    hi = lambda t: _frame_flip(t[split:], F)  # noqa: E731
    y_r, h_r = sm.scan_ref64(hi(i.u), hi(i.delta), pi.A_b, hi(i.B), hi(i.C), pi.D_b, hi(i.z),
                             pi.bias_b, True, pi.h0_b)
    y_f, h_ff = sm.scan_ref64(i.u[:split], i.delta[:split], i.A, i.B[:split], i.C[:split], i.D,
                              i.z[:split], i.bias, True, i.h0)
    assert torch.equal(y[split:], _frame_flip(y_r, F)) and torch.equal(h_b, h_r)
    assert torch.equal(y[:split], y_f) and torch.equal(h_f, h_ff)
    assert not torch.equal(pi.A_b, i.A) and not torch.equal(pi.h0_b, i.h0)
    if F == L:
        assert torch.equal(y[split:], y_r)
    if F == 1:
        assert torch.equal(y[split:], torch.flip(y_r, dims=[2]))


def test_option_table_is_a_covering_array():
    assert sm.covering_gaps(sm.ROWS) == []
    assert len(sm.ROWS) <= sm.MAX_ROWS
    assert len(set(sm.ROWS)) == len(sm.ROWS)


def test_covering_check_rejects_tables_with_gaps():
    """A hand-made table that misses a pair must fail: dropping any row of the table, a
    full factorial over the options with one state kind only, and a table that never has
    softplus off with z absent."""
    for k in range(len(sm.ROWS)):
        assert sm.covering_gaps(sm.ROWS[:k] + sm.ROWS[k + 1:]), k
    one_state = [sm.Row(bool(i & 1), bool(i & 2), bool(i & 4), bool(i & 8), "h0_hl")
                 for i in range(12)]
    assert any("state=" in g for g in sm.covering_gaps(one_state))
    no_pair = [r._replace(z=True) if not r.softplus else r for r in sm.ROWS]
    assert "z=False with softplus=False" in sm.covering_gaps(no_pair)
    assert sm.covering_gaps(sm.ROWS + sm.ROWS[:3])  # more than MAX_ROWS rows


# Shapes (and dtypes, seeds) the GPU matrix runs; the sensitivity floor must hold at each.
F32, BF16 = torch.float32, torch.bfloat16
SENS_CASES = [(s, 1, dt) for s in [(2, 136, 150, 16), (2, 136, 150, 8), (2, 136, 24, 16),
                                   (2, 136, 24, 8)] for dt in DTYPES]
# the paired cases' backward direction takes seed 1001
SENS_CASES += [(s, 1001, dt) for s in [(2, 136, 150, 16), (2, 136, 24, 16)] for dt in DTYPES]
# channel-major forms exist for one dtype each
SENS_CASES += [((2, 24, 300, 16), 1, F32), ((2, 24, 600, 16), 1, F32), ((2, 24, 1300, 16), 1, F32),
               ((2, 24, 300, 16), 1, BF16), ((1, 12, 600, 16), 1, BF16),
               ((1, 12, 1300, 16), 1, BF16), ((30, 72, 100, 16), 1, BF16),
               ((30, 72, 600, 16), 1, BF16), ((30, 72, 1300, 16), 1, BF16)]
FLOOR = 0.05


@pytest.mark.parametrize("shape,seed,dt", SENS_CASES,
                         ids=["x".join(map(str, s)) + f"-s{k}-{_dtid(d)}" for s, k, d in SENS_CASES])
@pytest.mark.parametrize("row", sm.ROWS, ids=lambda r: r.id)
def test_inputs_are_sensitive_to_every_operand(row, dt, shape, seed):
    """For every operand the row has, the reference recomputed without it (or with softplus
    flipped) must fail the GPU tests' comparator on at least 5 % of y, and for h0, bias and
    softplus on at least 5 % of h_last — a kernel that drops the operand cannot pass.  A
    condition on the inputs: if it fails, the inputs change, not the floor.  (At L = 24, the
    carry cases' length, h0 reaches every h_last element; with ``_rand_scan``'s inputs of
    test_gpu_parity.py the h0 -> h_last fraction at L = 150 is zero.)"""
    inp = sm.make_inputs(row, dt, *shape, seed=seed)
    y, h = inp.ref(row.softplus)
    y_cmp = sm.round_like(y, dt)
    tol_y, tol_h = sm.TOL_Y[dt], row.state_tol
    variants = {"softplus": inp.ref(not row.softplus)}
    for name in ("D", "z", "bias", "h0"):
        if getattr(inp, name) is not None:
            variants[name] = inp.ref(row.softplus, **{name: None})
    for name, (y2, h2) in variants.items():
        fy = sm.mismatch(sm.round_like(y2, dt), y_cmp, tol_y).double().mean().item()
        assert fy >= FLOOR, f"{name}: only {fy:.1%} of y changes beyond {tol_y:g}"
        if name in ("h0", "bias", "softplus"):
            fh = sm.mismatch(h2, h, tol_h).double().mean().item()
            assert fh >= FLOOR, f"{name}: only {fh:.1%} of h_last changes beyond {tol_h:g}"
