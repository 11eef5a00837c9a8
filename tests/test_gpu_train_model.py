"""``Block`` and ``PretrainVideoMamba`` in training mode are differentiable end to end: outputs,
every parameter gradient and the input gradients against autograd through the CPU oracle
(``oracle.block_forward`` / ``oracle.encoder_forward``) in fp32 on the same parameter values.

Bounds (relative L2 per tensor)
    fp32 models (TF32 off): <= 1e-4, the mixer test's bound.
    bf16 models: no fixed bound fits — the oracle's own bf16 CPU autograd at these shapes sits
    0.6e-2 to 1.4e-2 from its fp32 autograd (worst dt_proj.weight and x_proj.weight), so the
    project's 1e-2 would fail the reference itself.  Each bf16 case computes that distance
    d_k per gradient k on the CPU and requires the GPU gradient within max(1e-2, 3 d_k) of the
    fp32 oracle: two independently rounded bf16 computations differ by about sqrt(2) d_k and
    the kernels round in another order.  d_k and the achieved distance are printed.

Block: d_model 64, L 24, batch 2; fused RMSNorm + fp32 residual, fused LayerNorm + residual in
the model dtype (bf16 for the bf16 model), unfused; with and without ``state``.
Model: img 16, patch 8, embed 64, 4 frames, depth 2, batch 2 (17 tokens): plain cls+avg; masked
(6 of 17 hidden, another pattern per sample) with keep_temporal; avg + LayerNorm + model-dtype
residual; unfused cls_cat_avg; a 16 x 24 input (interpolated spatial embedding).  The loss is
a fixed random projection of x_vis plus one of x_pool.

Also: what the parent commit could not do (norm.weight.grad, gradients into earlier rows,
outputs that require grad, no "not differentiable" warning), the unchanged inference
behaviour (.eval(), no_grad, ssm_state: no graph, the no_grad call's bits, the warning), and
one SGD step that lowers an MSE loss.

Measured on the MI355X (relative L2, worst over every output and gradient of every case):
    fp32   3.6e-6 (model masked_keep_temporal, layers.0.mixer.x_proj.weight); most 2e-7 - 1e-6
    bf16   Block: 2.0e-4 - 8.7e-3 with d_k 2.0e-4 - 8.7e-3 — the GPU gradient sits as far from the
           fp32 oracle as the oracle's own bf16 run does (equal to three digits in most rows);
           model: 2.2e-3 - 3.4e-2 with d_k 2.2e-3 - 6.2e-2, the largest on
           layers.0.mixer.x_proj.weight (masked: 3.4e-2 at d_k 6.2e-2; plain: 2.3e-2 at 2.3e-2);
           the closest to its bound is layers.1.mixer.x_proj.weight of the masked case, 1.16e-2
           at d_k 9.2e-3: 0.42 of max(1e-2, 3 d_k).
"""

import warnings

import pytest
import torch

from oracle import videomamba_oracle as orc
from videomamba_amd import layers
from videomamba_amd.videomamba import PretrainVideoMamba, create_block

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-5


@pytest.fixture(autouse=True)
def _no_tf32():
    prev = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = prev


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for prm in m.parameters():
            prm.add_(0.02 * torch.randn(prm.shape, generator=g))
    return m


def _check(dt, what, got, ref32, ref_bf):
    """got: GPU values by name; ref32: the fp32 oracle's; ref_bf: the bf16 oracle's (bf16 models
    only).  Asserts the module docstring's bounds, prints every distance."""
    assert set(got) == set(ref32), (set(got) ^ set(ref32))
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
    print(f"\n{what}: " + " ".join(lines))
    assert not bad, bad


# ----------------------------------------------------------------------------- Block
BLOCK_KINDS = {"fused_rms_fp32res": dict(fused=True, rms=True, rif=True),
               "fused_ln_dtres": dict(fused=True, rms=False, rif=False),
               "unfused": dict(fused=False, rms=True, rif=True)}


def _block(kind, dt):
    kw = BLOCK_KINDS[kind]
    torch.manual_seed(7)
    b = create_block(64, norm_epsilon=EPS, rms_norm=kw["rms"], residual_in_fp32=kw["rif"],
                     fused_add_norm=kw["fused"], layer_idx=0)
    return _perturb(b, 8).to(dt).to(DEV).train()


def _block_inputs(dt, rif, stateful):
    g = torch.Generator().manual_seed(3)
    ins = {"hidden": torch.randn(2, 24, 64, generator=g).to(dt),
           "residual": torch.randn(2, 24, 64, generator=g).to(F32 if rif else dt)}
    if stateful:
        ins["conv_state"] = torch.randn(2, 128, 4, generator=g).to(dt)
        ins["ssm_state"] = torch.randn(2, 128, 16, generator=g)
    gs = {"hidden": torch.randn(2, 24, 64, generator=g),
          "residual": torch.randn(2, 24, 64, generator=g),
          "ssm": torch.randn(2, 128, 16, generator=g)}
    return ins, gs


def _oracle_block(params, ins, gs, kw, dt):
    """Autograd through oracle.block_forward on the CPU in ``dt``: outputs and gradients."""
    p = {k: v.detach().cpu().to(dt).requires_grad_(True) for k, v in params.items()}
    lv = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in ins.items()}  # own dtypes
    state = (lv["conv_state"], lv["ssm_state"]) if "ssm_state" in lv else None
    h, r, st = orc.block_forward(p, "", lv["hidden"], lv["residual"], fused=kw["fused"],
                                 residual_in_fp32=kw["rif"], is_rms=kw["rms"], eps=EPS,
                                 d_state=16, d_conv=4, state=state)
    loss = (h.float() * gs["hidden"]).sum() + (r.float() * gs["residual"]).sum()
    outs = {"hidden_out": h, "residual_out": r}
    if st is not None:
        loss = loss + (st[1].float() * gs["ssm"]).sum()
        outs["new_ssm"] = st[1]
    leaves = {**{"d" + k: v for k, v in p.items()}, **{"d" + k: v for k, v in lv.items()}}
    grads = torch.autograd.grad(loss, list(leaves.values()))
    return {**outs, **dict(zip(leaves, grads))}


@pytest.mark.parametrize("stateful", [False, True], ids=["stateless", "state"])
@pytest.mark.parametrize("kind", list(BLOCK_KINDS))
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
def test_training_block_gradients_match_the_oracle(dt, kind, stateful):
    kw = BLOCK_KINDS[kind]
    blk = _block(kind, dt)
    ins, gs = _block_inputs(dt, kw["rif"], stateful)
    params = {k: v.detach().cpu().float() for k, v in blk.state_dict().items()}  # dt-valued
    ins32 = {k: v.float() for k, v in ins.items()}
    ref32 = _oracle_block(params, ins32, gs, kw, F32)
    ref_bf = _oracle_block(params, ins, gs, kw, BF16) if dt == BF16 else None

    lv = {k: v.to(DEV).requires_grad_(True) for k, v in ins.items()}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        if stateful:
            h, r, (new_conv, new_ssm) = blk(lv["hidden"], lv["residual"],
                                            state=(lv["conv_state"], lv["ssm_state"]),
                                            return_state=True)
        else:
            h, r = blk(lv["hidden"], lv["residual"])
    assert not [w for w in caught if "not differentiable" in str(w.message)]
    assert h.requires_grad and r.requires_grad and h.dtype == dt
    assert r.dtype == (F32 if kw["rif"] else dt)
    loss = (h.float() * gs["hidden"].to(DEV)).sum() + (r.float() * gs["residual"].to(DEV)).sum()
    got = {"hidden_out": h, "residual_out": r}
    if stateful:
        loss = loss + (new_ssm * gs["ssm"].to(DEV)).sum()
        got["new_ssm"] = new_ssm
    leaves = {**{"d" + k: v for k, v in blk.named_parameters()},
              **{"d" + k: v for k, v in lv.items()}}
    grads = torch.autograd.grad(loss, list(leaves.values()))
    for (k, leaf), gr in zip(leaves.items(), grads):
        assert gr.shape == leaf.shape and gr.dtype == leaf.dtype, k
        got[k] = gr
    assert "dnorm.weight" in got
    _check(dt, f"block {kind} {dt} stateful={stateful}", got, ref32, ref_bf)


def test_training_block_moves_its_norm_and_passes_gradient_to_earlier_rows():
    """What the parent commit could not do: after backward norm.weight.grad exists, and the
    gradient reaches hidden_states and residual produced by an earlier layer."""
    first, second = _block("fused_rms_fp32res", F32), _block("fused_rms_fp32res", F32)
    x = torch.randn(2, 24, 64, device=DEV)
    h, r = first(x)
    h2, r2 = second(h, r)
    assert h2.requires_grad and r2.requires_grad
    (h2.square().sum() + r2.square().sum()).backward()
    for blk in (first, second):
        assert blk.norm.weight.grad is not None and float(blk.norm.weight.grad.abs().sum()) > 0
        assert all(p.grad is not None for p in blk.parameters())
    h, r = first(x)
    h.retain_grad(), r.retain_grad()
    h2, _ = second(h, r)
    h2.square().sum().backward()
    assert float(h.grad.abs().sum()) > 0 and float(r.grad.abs().sum()) > 0


# ----------------------------------------------------------------------------- model
MODEL_CASES = {
    "plain_cls+avg": dict(model=dict(pool_type="cls+avg")),
    "masked_keep_temporal": dict(model=dict(pool_type="cls+avg"), mask=True, keep_temporal=True),
    "avg_ln_dtres": dict(model=dict(pool_type="avg", rms_norm=False, residual_in_fp32=False)),
    "unfused_cls_cat_avg": dict(model=dict(pool_type="cls_cat_avg", fused_add_norm=False)),
    "nonsquare_16x24": dict(model=dict(pool_type="cls+avg"), hw=(16, 24)),
}


def _model(dt, **over):
    kw = dict(img_size=16, patch_size=8, depth=2, embed_dim=64, num_frames=4,
              norm_epsilon=EPS, fused_add_norm=True, rms_norm=True, residual_in_fp32=True,
              pool_type="cls+avg")
    kw.update(over)
    torch.manual_seed(5)
    m = _perturb(PretrainVideoMamba(**kw), 6).to(dt).to(DEV).train()
    cfg = dict(kw, kernel_size=1, d_state=16, d_conv=4)
    return m, cfg


def _mask():
    """(2, 17): 6 patch tokens hidden per sample, another pattern each, CLS and at least one
    token of each of the 4 frames (4 tokens per frame) visible."""
    m = torch.zeros(2, 17, dtype=torch.bool)
    m[0, [1, 2, 6, 9, 10, 15]] = True
    m[1, [3, 4, 5, 11, 13, 14]] = True
    return m


def _oracle_model(params, cfg, x, mask, keep_temporal, proj, dt):
    p = {k: v.detach().cpu().to(dt).requires_grad_(True) for k, v in params.items()}
    xv = x.detach().cpu().to(dt).requires_grad_(True)
    vis, pool, _ = orc.encoder_forward(p, cfg, xv, mask=mask, keep_temporal=keep_temporal)
    loss = (vis.float() * proj[0]).sum() + (pool.float() * proj[1]).sum()
    leaves = {**{"d" + k: v for k, v in p.items()}, "dvideo": xv}
    grads = torch.autograd.grad(loss, list(leaves.values()))
    return {"x_vis": vis, "x_pool": pool, **dict(zip(leaves, grads))}


@pytest.mark.parametrize("case", list(MODEL_CASES))
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
def test_training_model_gradients_match_the_oracle(dt, case):
    spec = MODEL_CASES[case]
    model, cfg = _model(dt, **spec["model"])
    H, W = spec.get("hw", (16, 16))
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, 4, H, W, generator=g).to(dt)
    mask = _mask() if spec.get("mask") else None
    kt = bool(spec.get("keep_temporal"))
    params = {k: v.detach().cpu().float() for k, v in model.state_dict().items()}
    with torch.no_grad():
        shapes = [t.shape for t in orc.encoder_forward(params, cfg, x.float(), mask=mask,
                                                       keep_temporal=kt)[:2]]
    proj = [torch.randn(s, generator=g) for s in shapes]
    ref32 = _oracle_model(params, cfg, x.float(), mask, kt, proj, F32)
    ref_bf = _oracle_model(params, cfg, x, mask, kt, proj, BF16) if dt == BF16 else None

    xd = x.to(DEV).requires_grad_(True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        vis, pool = model(xd, mask=None if mask is None else mask.to(DEV), keep_temporal=kt)
    assert not [w for w in caught if "not differentiable" in str(w.message)]
    assert vis.requires_grad and pool.requires_grad and vis.dtype == dt
    assert list(vis.shape) == list(shapes[0]) and list(pool.shape) == list(shapes[1])
    loss = (vis.float() * proj[0].to(DEV)).sum() + (pool.float() * proj[1].to(DEV)).sum()
    leaves = {**{"d" + k: v for k, v in model.named_parameters()}, "dvideo": xd}
    grads = torch.autograd.grad(loss, list(leaves.values()))
    got = {"x_vis": vis, "x_pool": pool}
    for (k, leaf), gr in zip(leaves.items(), grads):
        assert gr.shape == leaf.shape and gr.dtype == leaf.dtype, k
        got[k] = gr
    _check(dt, f"model {case} {dt}", got, ref32, ref_bf)


def test_forward_features_in_training_mode_is_differentiable():
    model, _ = _model(F32)
    x = torch.randn(2, 3, 4, 16, 16, device=DEV)
    feats = model.forward_features(x)
    vis, _ = model(x)
    assert feats.requires_grad and feats.shape == (2, 17, 64)
    assert torch.equal(feats[:, 1:], vis)


# ----------------------------------------------------------------------------- unchanged paths
def _warns(fn):
    layers._warned_grad = False  # the warning is raised once per process
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = fn()
    return out, bool([w for w in caught if "not differentiable" in str(w.message)])


def test_eval_no_grad_and_ssm_state_keep_the_inference_path():
    """.eval() with grad mode on, .train() under no_grad and .train() with ``ssm_state``: no
    graph, the bits of the no_grad call, and the warning where autograd would expect one."""
    model, _ = _model(F32)
    x = torch.randn(2, 3, 4, 16, 16, device=DEV)
    with torch.no_grad():
        ref_v, ref_p = model.eval()(x)
    (v, p), warned = _warns(lambda: model.eval()(x))
    assert warned and not v.requires_grad and not p.requires_grad
    assert torch.equal(v, ref_v) and torch.equal(p, ref_p)
    model.train()
    with torch.no_grad():
        (v, p), warned = _warns(lambda: model(x))
    assert not warned and not v.requires_grad and torch.equal(v, ref_v) and torch.equal(p, ref_p)
    # carried state: the model-level training path does not take it
    with torch.no_grad():
        rv, rp, _ = model(x, ssm_state=model.allocate_state(2, device=DEV))
    (v, p, st), warned = _warns(lambda: model(x, ssm_state=model.allocate_state(2, device=DEV)))
    assert warned and not v.requires_grad and not p.requires_grad
    assert torch.equal(v, rv) and torch.equal(p, rp)
    assert not any(t.requires_grad for pair in st for t in pair)


def test_eval_block_keeps_the_inference_path():
    blk = _block("fused_rms_fp32res", F32).eval()
    x = torch.randn(2, 24, 64, device=DEV)
    r = torch.randn(2, 24, 64, device=DEV)
    with torch.no_grad():
        ref_h, ref_r = blk(x, r)
    (h, r2), warned = _warns(lambda: blk(x, r))
    assert warned and not h.requires_grad and not r2.requires_grad
    assert torch.equal(h, ref_h) and torch.equal(r2, ref_r)
    blk.train()
    with torch.no_grad():
        h, r2 = blk(x, r)
    assert not h.requires_grad and torch.equal(h, ref_h) and torch.equal(r2, ref_r)
    # the legacy in-place ssm_state keeps the whole block on the inference path
    (h, r2), warned = _warns(lambda: blk(x, r, ssm_state=torch.zeros(2, 128, 16, device=DEV)))
    assert warned and not h.requires_grad and not r2.requires_grad and torch.equal(r2, ref_r)


# ----------------------------------------------------------------------------- training step
def test_one_sgd_step_lowers_the_loss():
    model, _ = _model(F32)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 4, 16, 16, generator=g).to(DEV)
    target = torch.randn(2, 1, 64, generator=g).to(DEV)
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    loss0 = torch.nn.functional.mse_loss(model(x)[1], target)
    opt.zero_grad()
    loss0.backward()
    for name, prm in model.named_parameters():
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), name
    opt.step()
    with torch.no_grad():
        loss1 = torch.nn.functional.mse_loss(model(x)[1], target)
    assert float(loss1) < float(loss0.detach()), (float(loss0.detach()), float(loss1))
