"""Training-path microbenchmark at VideoMamba-M / 8 frames geometry (d_model 576, d_inner 1152,
L = 1569, depth 32, bf16); prints one JSON line.

Times forward + backward, per batch (default 8 and 32), with device events after a warm-up,
each once on the HIP kernels (``options.train_ops = "hip"``: vm_causal_conv1d_fwd / _bwd,
vm_add_norm_fwd / _bwd) and once on torch ops under autograd (``"torch"``):
  conv    depthwise conv + SiLU of one mixer, against the fp32 tap loop ``Mamba._forward_train``
          ran before the HIP backward existed
  norm    add + RMSNorm of one block (bf16 x, fp32 residual, both returns carrying gradient),
          against the same arithmetic as fp32 torch ops on the GPU
  block   one training ``Block``
  model   the 32-layer ``PretrainVideoMamba``
``--compare gemm`` (the default since ABI v17) keeps ``train_ops = "hip"`` on both sides and runs
each leg once with ``options.train_gemm = "hip"`` (in_proj / out_proj through
``kernels.linear_fn``: vm_linear_fwd, vm_linear_dgrad, vm_linear_wgrad) and once with
``"library"`` (``F.linear``, library GEMMs under autograd):
  in_proj   forward + backward of one 576 -> 2304 projection of batch x 1569 rows
  out_proj  the same for 1152 -> 576
  block, model  as above
``--compare ops`` is the comparison described first (conv, norm, block, model).
``--compare refiner`` (ABI v19) times one training ``BiMambaRefinerBlock`` (C = 576, a
(B, 8, 196, 576) input, B = 1, 2, 4, 8 by default) once with ``options.train_refiner = "paired"``
(one vm_selective_scan_bidir_bwd launch over the 2 B rows of both directions) and once with
``"blocks"`` (the composition on the differentiable ``Block``: two vm_selective_scan_bwd launches
of B rows); ``verdict`` then carries, per batch, both medians and the larger min-to-max spread.
Every measurement runs in a child process of its own under a time limit, so a slow leg cannot
hold the device for minutes.  ``verdict`` says, per leg and batch, whether the HIP median is
within the other side's median plus the larger min-to-max spread of the two.

    python scripts/bench_train_bwd.py [--batches 8 32] [--reps 20] > profiles/train_bwd_<tag>.json
    python scripts/bench_train_bwd.py --compare refiner > profiles/train_refiner_<tag>.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DMODEL, DIM, SEQLEN, WIDTH, DEPTH, FRAMES = 576, 1152, 1569, 4, 32, 8
LEGS = ("conv", "norm", "in_proj", "out_proj", "block", "model", "refiner")
REFINER_TOKENS, REFINER_BATCHES = 196, (1, 2, 4, 8)  # (B, FRAMES, 196, DMODEL) inputs
COMPARE = {"ops": (("conv", "norm", "block", "model"), "torch"),
           "gemm": (("in_proj", "out_proj", "block", "model"), "library")}
PROJ = {"in_proj": (2 * DIM, DMODEL), "out_proj": (DMODEL, DIM)}  # (n, k)


def _time(fn, warmup, reps):
    """Per-call device-event times in microseconds."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    us = [1e3 * a.elapsed_time(b) for a, b in pairs]
    return dict(median=round(statistics.median(us), 1), min=round(min(us), 1),
                max=round(max(us), 1), mean=round(statistics.fmean(us), 1))


def _conv(batch, ops, gemm, dev):
    import torch
    import torch.nn.functional as F
    from videomamba_amd import kernels as K
    g = torch.Generator().manual_seed(batch)
    x = torch.randn(batch, SEQLEN, DIM, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    w = (0.5 * torch.randn(DIM, WIDTH, generator=g)).to(dev).requires_grad_(True)
    b = (0.5 * torch.randn(DIM, generator=g)).to(dev).requires_grad_(True)
    dout = torch.randn(batch, SEQLEN, DIM, generator=g).to(torch.bfloat16).to(dev)

    def hip():
        u = K.causal_conv1d_fn(x.transpose(1, 2), w, b, "silu").transpose(1, 2)
        torch.autograd.grad(u, [x, w, b], dout)

    def taps():  # the tap loop of Mamba._forward_train
        xin = torch.cat([x.new_zeros((batch, WIDTH, DIM)), x], dim=1)
        xf = xin.float()
        acc = xf[:, 1:1 + SEQLEN] * w[:, 0]
        for k in range(1, WIDTH):
            acc = acc + xf[:, 1 + k:1 + k + SEQLEN] * w[:, k]
        u = F.silu(acc + b).to(x.dtype)
        torch.autograd.grad(u, [x, w, b], dout)

    return hip if ops == "hip" else taps


def _norm(batch, ops, gemm, dev):
    import torch
    from videomamba_amd import kernels as K, options
    g = torch.Generator().manual_seed(batch)
    rows = batch * SEQLEN
    x = torch.randn(rows, DMODEL, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    r = torch.randn(rows, DMODEL, generator=g).to(dev).requires_grad_(True)
    w = (1.0 + 0.1 * torch.randn(DMODEL, generator=g)).to(dev).requires_grad_(True)
    gy = torch.randn(rows, DMODEL, generator=g).to(torch.bfloat16).to(dev)
    gs = torch.randn(rows, DMODEL, generator=g).to(dev)

    def pair():
        with options.override(train_ops=ops):
            y, s = K.rms_norm_fn(x, w, None, residual=r, prenorm=True, residual_in_fp32=True,
                                 eps=1e-5)
        torch.autograd.grad([y, s], [x, r, w], [gy, gs])

    return pair


def _proj(leg):
    def make(batch, ops, gemm, dev):
        import torch
        from videomamba_amd import kernels as K, options
        n, k = PROJ[leg]
        g = torch.Generator().manual_seed(batch)
        x = torch.randn(batch, SEQLEN, k, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
        w = (torch.randn(n, k, generator=g) * k ** -0.5).to(torch.bfloat16).to(dev).requires_grad_(True)
        gy = torch.randn(batch, SEQLEN, n, generator=g).to(torch.bfloat16).to(dev)

        def pair():
            with options.override(train_gemm=gemm):
                y = K.linear_fn(x, w)
            torch.autograd.grad(y, [x, w], gy)

        return pair
    return make


def _block(batch, ops, gemm, dev):
    import torch
    from videomamba_amd import options
    from videomamba_amd.videomamba import create_block
    torch.manual_seed(0)
    blk = create_block(DMODEL, layer_idx=0).to(torch.bfloat16).to(dev).train()
    g = torch.Generator().manual_seed(batch)
    h = torch.randn(batch, SEQLEN, DMODEL, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    r = torch.randn(batch, SEQLEN, DMODEL, generator=g).to(dev).requires_grad_(True)
    gh = torch.randn(batch, SEQLEN, DMODEL, generator=g).to(torch.bfloat16).to(dev)
    gr = torch.randn(batch, SEQLEN, DMODEL, generator=g).to(dev)
    leaves = [h, r] + list(blk.parameters())

    def pair():
        with options.override(train_ops=ops, train_gemm=gemm):
            ho, ro = blk(h, r)
            torch.autograd.grad([ho, ro], leaves, [gh, gr])

    return pair


def _model(batch, ops, gemm, dev):
    import torch
    from videomamba_amd import options
    from videomamba_amd.videomamba import PretrainVideoMamba
    torch.manual_seed(0)
    model = PretrainVideoMamba(depth=DEPTH, embed_dim=DMODEL, num_frames=FRAMES,
                               pool_type="cls+avg").to(torch.bfloat16).to(dev).train()
    g = torch.Generator().manual_seed(batch)
    x = torch.randn(batch, 3, FRAMES, 224, 224, generator=g).to(torch.bfloat16).to(dev)

    def pair():
        model.zero_grad(set_to_none=True)
        with options.override(train_ops=ops, train_gemm=gemm):
            vis, pool = model(x)
            (pool.float().square().mean() + vis.float().square().mean()).backward()

    return pair


def _refiner(batch, mode, dev):
    import torch
    from videomamba_amd import options
    from videomamba_amd.refiner_backbone import BiMambaRefinerBlock
    torch.manual_seed(0)
    blk = BiMambaRefinerBlock(DMODEL, layer_idx=0).to(torch.bfloat16).to(dev).train()
    g = torch.Generator().manual_seed(batch)
    shape = (batch, FRAMES, REFINER_TOKENS, DMODEL)
    x = torch.randn(*shape, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    gy = torch.randn(*shape, generator=g).to(torch.bfloat16).to(dev)
    leaves = [x] + list(blk.parameters())

    def pair():
        with options.override(train_refiner=mode):
            out, _ = blk(x)
            torch.autograd.grad(out, leaves, gy)

    return pair


def child(leg, batch, ops, gemm, warmup, reps, refiner="paired"):
    import torch
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda", 0)
    if leg == "refiner":
        t = _time(_refiner(batch, refiner, dev), warmup, reps)
        return dict(leg=leg, batch=batch, refiner=refiner, fwd_bwd_us=t,
                    peak_mem_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20))
    fn = {"conv": _conv, "norm": _norm, "in_proj": _proj("in_proj"), "out_proj": _proj("out_proj"),
          "block": _block, "model": _model}[leg](batch, ops, gemm, dev)
    t = _time(fn, warmup, reps)
    return dict(leg=leg, batch=batch, ops=ops, gemm=gemm, fwd_bwd_us=t,
                peak_mem_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20))


def _main_refiner(a):
    """``--compare refiner``: "paired" against "blocks" per batch, a child process each."""
    out = dict(bench="train_bwd", compare="refiner", d_model=DMODEL, d_inner=DIM,
               seqlen=FRAMES * REFINER_TOKENS, frames=FRAMES, dtype="bf16", reps=a.reps,
               warmup=a.warmup, timer="device events", results=[], verdict=[])
    for b in a.batches or REFINER_BATCHES:
        pair = {}
        for mode in ("paired", "blocks"):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__),
                   "--child", "refiner", "--batch", str(b), "--refiner", mode,
                   "--reps", str(a.reps), "--warmup", str(a.warmup)]
            run = subprocess.run(cmd, capture_output=True, text=True)
            if run.returncode != 0:  # a faulted or hung leg: start nothing more on the device
                out["results"].append(dict(leg="refiner", batch=b, refiner=mode,
                                           error=f"exit {run.returncode}",
                                           stderr=run.stderr[-400:]))
                print(json.dumps(out), flush=True)
                return 1
            r = json.loads(run.stdout.strip().splitlines()[-1])
            out["results"].append(r)
            pair[mode] = r["fwd_bwd_us"]
        spread = max(p["max"] - p["min"] for p in pair.values())
        pm, bm = pair["paired"]["median"], pair["blocks"]["median"]
        out["verdict"].append({
            "leg": "refiner", "batch": b, "paired_us": pm, "blocks_us": bm,
            "spread_us": round(spread, 1), "blocks_over_paired": round(bm / pm, 2),
            "paired_faster_beyond_spread": pm < bm - spread,
            "paired_not_slower": pm <= bm + spread})
    print(json.dumps(out), flush=True)
    return 0


def _run_child(leg, batch, ops, gemm, a):
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__),
           "--child", leg, "--batch", str(batch), "--ops", ops, "--gemm", gemm,
           "--reps", str(a.reps), "--warmup", str(a.warmup)]
    run = subprocess.run(cmd, capture_output=True, text=True)
    if run.returncode != 0:
        return dict(leg=leg, batch=batch, ops=ops, gemm=gemm, error=f"exit {run.returncode}",
                    stderr=run.stderr[-400:])
    return json.loads(run.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=None,
                    help="default 8 32 (--compare refiner: 1 2 4 8)")
    ap.add_argument("--compare", choices=list(COMPARE) + ["refiner"], default="gemm")
    ap.add_argument("--legs", nargs="+", choices=LEGS, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", choices=LEGS)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--ops", choices=["hip", "torch"], default="hip")
    ap.add_argument("--gemm", choices=["hip", "library"], default="library")
    ap.add_argument("--refiner", choices=["paired", "blocks"], default="paired")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    if a.child:
        print(json.dumps(child(a.child, a.batch, a.ops, a.gemm, a.warmup, a.reps, a.refiner)),
              flush=True)
        return 0
    if a.compare == "refiner":
        return _main_refiner(a)
    a.batches = a.batches or [8, 32]
    legs, other = COMPARE[a.compare]
    legs = [leg for leg in (a.legs or legs) if leg in legs]
    out = dict(bench="train_bwd", compare=a.compare, d_model=DMODEL, d_inner=DIM, seqlen=SEQLEN, depth=DEPTH,
               dtype="bf16", reps=a.reps, warmup=a.warmup, timer="device events", results=[],
               verdict=[])
    for leg in legs:
        for b in a.batches:
            pair = {}
            for side in ("hip", other):
                # the side varies train_ops ("ops") or train_gemm ("gemm"); the ops comparison
                # keeps the parent's GEMM path, the gemm comparison keeps train_ops = "hip"
                ops, gemm = (side, "library") if a.compare == "ops" else ("hip", side)
                r = _run_child(leg, b, ops, gemm, a)
                out["results"].append(r)
                if "error" in r:  # a faulted or hung leg: start nothing more on the device
                    print(json.dumps(out), flush=True)
                    return 1
                pair[side] = r["fwd_bwd_us"]
            spread = max(p["max"] - p["min"] for p in pair.values())
            out["verdict"].append({
                "leg": leg, "batch": b, "hip_us": pair["hip"]["median"],
                other + "_us": pair[other]["median"], "spread_us": round(spread, 1),
                other + "_over_hip": round(pair[other]["median"] / pair["hip"]["median"], 2),
                "hip_not_slower": pair["hip"]["median"] <= pair[other]["median"] + spread})
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
