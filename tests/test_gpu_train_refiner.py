"""``BiMambaRefinerBlock`` in training mode is differentiable end to end, on both of its
training paths (``options.train_refiner``: "paired" — one ``selective_scan_bidir_fn`` call, its
backward one ``vm_selective_scan_bidir_bwd`` launch — and "blocks", the reference's composition
on the differentiable ``Block``): the output, the new forward state, every parameter gradient
of both blocks, the gate and the Linear, the input gradient and the state gradients against
autograd through the CPU oracle (``oracle.refiner_forward``) in fp32 on the same parameter
values.

Bounds (relative L2 per tensor), those of test_gpu_train_model.py
    fp32 (TF32 off): <= 1e-4.
    bf16: within max(1e-2, 3 d_k) of the fp32 oracle, d_k the oracle's own bf16-vs-fp32
    distance for that tensor, computed here and printed with the achieved distance.
    fp32 "paired" against fp32 "blocks": <= 1e-5 (the same arithmetic: the scan backward's bits
    are equal, the paired forward is another kernel form than the plain forward).

C = 64 (d_inner 128), batch 2: a 3-D (2, 24, 64) input; 4-D (2, 3, 8, 64) and (2, 3, 7, 64)
inputs (frames reversed whole; L = 21 is no multiple of the 8-step chunk); fused RMSNorm and
fused LayerNorm blocks; without states, with states, and with states that require grad.

Also: what the parent commit could not do (every parameter has a ``.grad``, the output
requires grad, no "not differentiable" warning, one SGD step lowers an MSE loss), the
unchanged inference behaviour (``.eval()`` and ``no_grad``: no graph, ssm states updated in
place, the warning) and ``d_state = 8`` raising the mixer's ``NotImplementedError``.

Measured on the MI355X (relative L2, worst over every output and gradient of every case, the
same on both paths to three digits):
    fp32   2.2e-6 (block_bwd.mixer.A_log, 4-D 3 x 7); most 1e-7 - 1e-6
    bf16   3.8e-5 - 9.5e-3 with d_k 3.8e-5 - 9.6e-3: the GPU gradient sits as far from the fp32
           oracle as the oracle's own bf16 run does; the closest to its bound is
           fusion_gate.0.bias of the 3-D LayerNorm case, 6.7e-3 at d_k 5.4e-3 (0.41 of the bound)
    paired vs blocks, fp32: 0 on everything but block_bwd.mixer.out_proj.weight (1.4e-7 - 1.6e-7)
"""

import warnings

import pytest
import torch

from oracle import videomamba_oracle as orc
from videomamba_amd import layers, options
from videomamba_amd.refiner_backbone import BiMambaRefinerBlock

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-5
C, DI = 64, 128
MODES = ["paired", "blocks"]

KINDS = {"fused_rms": dict(fused=True, rms=True, rif=True),
         "fused_ln": dict(fused=True, rms=False, rif=False)}
# name -> (input shape, block kind, states: None / "given" / "grad")
CASES = {
    "3d_rms": ((2, 24, C), "fused_rms", None),
    "4d_3x8_rms_states": ((2, 3, 8, C), "fused_rms", "given"),
    "4d_3x7_ln_state_grads": ((2, 3, 7, C), "fused_ln", "grad"),
    "3d_ln": ((2, 24, C), "fused_ln", None),
}
STATE_NAMES = ("state_fwd_conv", "state_fwd_ssm", "state_bwd_conv", "state_bwd_ssm")

_ORACLE = {}  # (case, model dtype, run dtype) -> the oracle's outputs and gradients
_GPU = {}     # (case, dtype, mode) -> the GPU's


@pytest.fixture(autouse=True)
def _no_tf32():
    prev = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = prev


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _refiner(kind, dt, **over):
    kw = KINDS[kind]
    torch.manual_seed(7)
    blk = BiMambaRefinerBlock(C, layer_idx=0, norm_epsilon=EPS, rms_norm=kw["rms"],
                              residual_in_fp32=kw["rif"], fused_add_norm=kw["fused"], **over)
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for prm in blk.parameters():
            prm.add_(0.02 * torch.randn(prm.shape, generator=g))
    return blk.to(dt).to(DEV).train()


def _inputs(case, dt):
    """x in ``dt``, the four states (conv in ``dt``, ssm fp32) or None, and the fixed random
    projections that make the loss."""
    shape, _, states = CASES[case]
    g = torch.Generator().manual_seed(3)
    ins = {"x": torch.randn(*shape, generator=g).to(dt)}
    if states:
        for k in STATE_NAMES:
            last = 4 if k.endswith("conv") else 16
            t = 0.5 * torch.randn(2, DI, last, generator=g)
            ins[k] = t.to(dt) if k.endswith("conv") else t
    gs = {"out": torch.randn(*shape, generator=g), "ssm": torch.randn(2, DI, 16, generator=g)}
    return ins, gs


def _pairs(lv):
    if "state_fwd_ssm" not in lv:
        return None, None
    return ((lv["state_fwd_conv"], lv["state_fwd_ssm"]),
            (lv["state_bwd_conv"], lv["state_bwd_ssm"]))


def _oracle(case, model_dt, dt, params):
    """Autograd through oracle.refiner_forward on the CPU in ``dt`` on the ``model_dt`` case's
    values (inputs in their own dtypes, cast to fp32 for the fp32 run)."""
    key = (case, model_dt, dt)
    if key not in _ORACLE:
        _, kind, states = CASES[case]
        kw = KINDS[kind]
        ins, gs = _inputs(case, model_dt)
        if dt == F32:
            ins = {k: v.float() for k, v in ins.items()}
        p = {k: v.detach().cpu().to(dt).requires_grad_(True) for k, v in params.items()}
        lv = {k: v.detach().clone().requires_grad_(True) for k, v in ins.items()}
        st_f, st_b = _pairs(lv)
        out, (nc, ns) = orc.refiner_forward(p, lv["x"], state_fwd=st_f, state_bwd_init=st_b,
                                            fused=kw["fused"], residual_in_fp32=kw["rif"],
                                            is_rms=kw["rms"], eps=EPS, d_state=16, d_conv=4)
        loss = (out.float() * gs["out"]).sum() + (ns.float() * gs["ssm"]).sum()
        leaves = {**{"d" + k: v for k, v in p.items()}, "dx": lv["x"]}
        if states == "grad":
            leaves.update({"d" + k: lv[k] for k in STATE_NAMES})
        grads = torch.autograd.grad(loss, list(leaves.values()))
        _ORACLE[key] = {"out": out, "new_conv": nc, "new_ssm": ns, **dict(zip(leaves, grads))}
    return _ORACLE[key]


def _gpu(case, dt, mode):
    key = (case, dt, mode)
    if key in _GPU:
        return _GPU[key]
    shape, kind, states = CASES[case]
    blk = _refiner(kind, dt)
    ins, gs = _inputs(case, dt)
    lv = {k: v.to(DEV).requires_grad_(k == "x" or states == "grad") for k, v in ins.items()}
    before = {k: v.detach().clone() for k, v in lv.items()}
    st_f, st_b = _pairs(lv)
    with warnings.catch_warnings(record=True) as caught, options.override(train_refiner=mode):
        warnings.simplefilter("always")
        out, (nc, ns) = blk(lv["x"], state_fwd=st_f, state_bwd_init=st_b, use_checkpoint=True)
    assert not [w for w in caught if "not differentiable" in str(w.message)]
    assert out.requires_grad and ns.requires_grad and out.dtype == dt and out.shape == shape
    assert nc.shape == (2, DI, 4) and ns.shape == (2, DI, 16) and ns.dtype == F32
    loss = (out.float() * gs["out"].to(DEV)).sum() + (ns.float() * gs["ssm"].to(DEV)).sum()
    leaves = {**{"d" + k: v for k, v in blk.named_parameters()}, "dx": lv["x"]}
    if states == "grad":
        leaves.update({"d" + k: lv[k] for k in STATE_NAMES})
    grads = torch.autograd.grad(loss, list(leaves.values()))
    got = {"out": out, "new_conv": nc, "new_ssm": ns}
    for (k, leaf), gr in zip(leaves.items(), grads):
        assert gr.shape == leaf.shape and gr.dtype == leaf.dtype, k
        got[k] = gr
    # the states are inputs: read, never modified, and the new state is not one of them
    for k, v in lv.items():
        assert torch.equal(v.detach(), before[k]), f"{k} was modified in training"
    if states:
        assert ns is not lv["state_fwd_ssm"] and nc is not lv["state_fwd_conv"]
    params = {k: v.detach().cpu().float() for k, v in blk.state_dict().items()}  # dt-valued
    _GPU[key] = (got, params)
    return _GPU[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
def test_training_refiner_matches_the_oracle(dt, case, mode):
    got, params = _gpu(case, dt, mode)
    ref32 = _oracle(case, dt, F32, params)
    ref_bf = _oracle(case, dt, BF16, params) if dt == BF16 else None
    assert set(got) == set(ref32), set(got) ^ set(ref32)
    for k in ("block_fwd.norm.weight", "block_bwd.mixer.A_log", "fusion_gate.0.weight",
              "out_proj.bias"):
        assert "d" + k in got
    bad, lines = {}, []
    for k in got:
        e = _rel(got[k], ref32[k])
        if dt == F32:
            bound, d = 1e-4, None
        else:
            d = _rel(ref_bf[k], ref32[k])
            bound = max(1e-2, 3.0 * d)
        lines.append(f"{k}={e:.2e}" + ("" if d is None else f"(d={d:.2e})"))
        if not e <= bound:
            bad[k] = (e, bound)
    print(f"\nrefiner {case} {dt} {mode}: " + " ".join(lines))
    assert not bad, bad


@pytest.mark.parametrize("case", list(CASES))
def test_paired_and_blocks_agree_in_fp32(case):
    a, _ = _gpu(case, F32, "paired")
    b, _ = _gpu(case, F32, "blocks")
    assert set(a) == set(b)
    worst = {k: _rel(a[k], b[k]) for k in a}
    print(f"\nrefiner {case} paired vs blocks: " + " ".join(f"{k}={v:.1e}" for k, v in worst.items()))
    assert all(v <= 1e-5 for v in worst.values()), {k: v for k, v in worst.items() if not v <= 1e-5}


def test_paired_path_runs_the_paired_scan(monkeypatch):
    """"paired" goes through kernels.selective_scan_bidir_fn (once per forward), "blocks"
    never does."""
    from videomamba_amd import kernels as K
    calls = []
    real = K.selective_scan_bidir_fn
    monkeypatch.setattr(K, "selective_scan_bidir_fn",
                        lambda *a, **k: (calls.append(a[0].shape), real(*a, **k))[1])
    blk = _refiner("fused_rms", F32)
    x = torch.randn(2, 3, 8, C, device=DEV)
    with options.override(train_refiner="paired"):
        out, _ = blk(x)
    assert calls == [(4, DI, 24)] and out.grad_fn is not None
    with options.override(train_refiner="blocks"):
        blk(x)
    assert len(calls) == 1


# ----------------------------------------------------------------------------- new ground
@pytest.mark.parametrize("mode", MODES)
def test_every_parameter_gets_a_gradient_and_a_step_lowers_the_loss(mode):
    """What the parent commit could not do: the output requires grad, no warning, every
    parameter has a finite ``.grad`` after backward, and one SGD step lowers an MSE loss."""
    blk = _refiner("fused_rms", F32)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 8, C, generator=g).to(DEV)
    target = torch.randn(2, 3, 8, C, generator=g).to(DEV)
    opt = torch.optim.SGD(blk.parameters(), lr=1e-3)
    layers._warned_grad = False
    with options.override(train_refiner=mode):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            out, _ = blk(x)
        assert not [w for w in caught if "not differentiable" in str(w.message)]
        assert out.requires_grad
        loss0 = torch.nn.functional.mse_loss(out, target)
        opt.zero_grad()
        loss0.backward()
        for name, prm in blk.named_parameters():
            assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), name
            assert float(prm.grad.abs().sum()) > 0, name
        opt.step()
        with torch.no_grad():
            loss1 = torch.nn.functional.mse_loss(blk(x)[0], target)
    assert float(loss1) < float(loss0.detach()), (float(loss0.detach()), float(loss1))


def test_d_state_8_raises_in_training():
    blk = _refiner("fused_rms", F32, ssm_cfg={"d_state": 8})
    assert blk.block_fwd.mixer.d_state == 8
    x = torch.randn(2, 24, C, device=DEV)
    for mode in MODES:
        with options.override(train_refiner=mode), pytest.raises(NotImplementedError):
            blk(x)
    with torch.no_grad():  # the inference path still takes it
        out, _ = blk(x)
    assert out.shape == x.shape


# ----------------------------------------------------------------------------- unchanged paths
def _warns(fn):
    layers._warned_grad = False  # the warning is raised once per process
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = fn()
    return out, bool([w for w in caught if "not differentiable" in str(w.message)])


def test_eval_and_no_grad_keep_the_inference_path():
    """.eval() with grad mode on and .train() under no_grad: no graph, the no_grad call's
    bits, the forward ssm state updated in place, and the warning where autograd would expect
    a graph.  The training forward computes the same function (1e-4 in fp32)."""
    blk = _refiner("fused_rms", F32)
    x = torch.randn(2, 3, 8, C, device=DEV)

    def states():
        g = torch.Generator().manual_seed(11)
        mk = lambda last: (0.3 * torch.randn(2, DI, last, generator=g)).to(DEV)  # noqa: E731
        return (mk(4), mk(16)), (mk(4), mk(16))

    st_f, st_b = states()
    ssm_before = st_f[1].clone()
    with torch.no_grad():
        ref, (rc, rs) = blk.eval()(x, state_fwd=st_f, state_bwd_init=st_b)
    assert rs is st_f[1] and not torch.equal(rs, ssm_before)  # updated in place
    st_f, st_b = states()
    (out, (nc, ns)), warned = _warns(lambda: blk.eval()(x, state_fwd=st_f, state_bwd_init=st_b))
    assert warned and not out.requires_grad and not ns.requires_grad and ns is st_f[1]
    assert torch.equal(out, ref) and torch.equal(nc, rc) and torch.equal(ns, rs)
    blk.train()
    st_f, st_b = states()
    with torch.no_grad():
        (out, (nc, ns)), warned = _warns(lambda: blk(x, state_fwd=st_f, state_bwd_init=st_b))
    assert not warned and not out.requires_grad and ns is st_f[1]
    assert torch.equal(out, ref) and torch.equal(ns, rs)
    for mode in MODES:
        st_f, st_b = states()
        with options.override(train_refiner=mode):
            out, (nc, ns) = blk(x, state_fwd=st_f, state_bwd_init=st_b)
        assert out.requires_grad and ns is not st_f[1] and torch.equal(st_f[1], ssm_before)
        assert _rel(out, ref) <= 1e-4 and _rel(ns, rs) <= 1e-4 and _rel(nc, rc) <= 1e-4, mode
