"""CPU tests: public API / streaming contract / builder / loader, mirroring the reference's
CPU tests (tests/test_public_api_contract.py, tests/test_videomamba_regressions.py), plus
the C-ABI library load + export check.  No kernel compute happens here (no GPU)."""

import ctypes
import json
import os
import re
import shutil
import subprocess
from types import SimpleNamespace
from typing import Any

import pytest
import torch

import video_mamba
import videomamba_amd.videomamba as vm_module
from videomamba_amd import _lib
from videomamba_amd.mamba_simple import Mamba
from videomamba_amd.videomamba import PretrainVideoMamba, create_block, load_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small_model(**overrides: Any) -> PretrainVideoMamba:
    kwargs: dict = dict(img_size=8, patch_size=4, depth=2, embed_dim=16, channels=3,
                        ssm_cfg={"use_fast_path": False}, fused_add_norm=False, rms_norm=False,
                        residual_in_fp32=False, kernel_size=1, num_frames=4)
    kwargs.update(overrides)
    return PretrainVideoMamba(**kwargs)


def _cfg(**over):
    base = dict(img_size=8, patch_size=4, depth=2, embed_dim=16, channels=3,
                drop_path_rate=0.0, ssm_cfg={"use_fast_path": False}, norm_epsilon=1e-5,
                fused_add_norm=False, rms_norm=False, residual_in_fp32=False, bimamba=True,
                pool_type="cls+avg", kernel_size=1, num_frames=4, use_checkpoint=False,
                checkpoint_num=0, pretrained=None, ckpt_num_frame=4)
    base.update(over)
    return SimpleNamespace(vision_encoder=SimpleNamespace(**base))


# ------------------------------------------------------------------ public API contract
def test_public_all_matches_reference_surface():
    assert set(video_mamba.__all__) == {
        "DeterminismConfig", "ForwardReturnSemantics", "LayerState", "BiMambaRefinerBlock",
        "PretrainVideoMamba", "STREAMING_CONTRACT_VERSION", "StateShape", "StreamingState",
        "add_determinism_args", "allocate_state", "build_videomamba", "configure_determinism",
        "configure_determinism_from_args", "expected_state_shapes", "forward_return_semantics",
        "model_forward_return_semantics", "validate_state"}
    for name in video_mamba.__all__:
        assert hasattr(video_mamba, name)
    assert video_mamba.build_videomamba is vm_module.build_videomamba
    from video_mamba.mamba_simple import Mamba as M2
    assert M2 is Mamba


def test_streaming_contract_allocate_and_validate_cpu():
    model = _small_model()
    state = video_mamba.allocate_state(model, batch_size=2, dtype=torch.float32)
    video_mamba.validate_state(model, state, batch_size=2)
    shapes = video_mamba.expected_state_shapes(model, batch_size=2)
    assert len(shapes) == model.depth
    assert shapes[0].conv_state == (2, model.layers[0].mixer.d_inner, 4)
    assert shapes[0].ssm_state == (2, model.layers[0].mixer.d_inner, 16)
    st_d = video_mamba.allocate_state(model, batch_size=2, as_dict=True)
    video_mamba.validate_state(model, st_d, batch_size=2)
    assert model.expected_state_shapes(2) == shapes


def test_validate_state_error_messages():
    model = _small_model()
    state = video_mamba.allocate_state(model, batch_size=1)
    with pytest.raises(ValueError, match="State length mismatch"):
        video_mamba.validate_state(model, state[:1], batch_size=1)
    with pytest.raises(ValueError, match="State dict keys mismatch"):
        video_mamba.validate_state(model, {0: state[0]}, batch_size=1)
    with pytest.raises(TypeError, match="list, tuple, or dict"):
        video_mamba.validate_state(model, "nope", batch_size=1)
    with pytest.raises(ValueError, match="conv_state shape mismatch"):
        video_mamba.validate_state(model, state, batch_size=2)
    with pytest.raises(ValueError, match="batch_size must be a positive integer"):
        video_mamba.expected_state_shapes(model, 0)
    with pytest.raises(TypeError, match="2-tuple"):
        video_mamba.validate_state(model, [state[0][0], state[1][0]], batch_size=1)


def test_model_contract_metadata_and_forward_semantics():
    model = _small_model(add_pool_norm=True)
    assert model.streaming_contract_version == video_mamba.STREAMING_CONTRACT_VERSION == "1.0.0"
    sem = model.forward_return_semantics()
    assert sem.without_state == "(x_vis, x_pool)"
    assert sem.with_state == "(x_vis, x_pool, next_state)"
    sem2 = _small_model(add_pool_norm=False).forward_return_semantics()
    assert sem2.without_state == "x_vis"
    assert sem2.with_state == "(x_vis, next_state)"
    assert video_mamba.model_forward_return_semantics(model) == sem


def test_configure_determinism_reseeds_torch_rng():
    video_mamba.configure_determinism(seed=1234, deterministic=True)
    x1 = torch.randn(8)
    video_mamba.configure_determinism(seed=1234, deterministic=True)
    x2 = torch.randn(8)
    torch.testing.assert_close(x1, x2)
    torch.use_deterministic_algorithms(False)


def test_determinism_cli_roundtrip():
    import argparse
    p = video_mamba.add_determinism_args(argparse.ArgumentParser())
    args = p.parse_args(["--seed", "7", "--deterministic", "--cudnn-benchmark", "off"])
    cfg = video_mamba.configure_determinism_from_args(args)
    assert cfg.seed == 7 and cfg.deterministic and not cfg.cudnn_benchmark and not cfg.allow_tf32
    torch.use_deterministic_algorithms(False)


# ------------------------------------------------------------------ builder / loader
def test_bimamba_false_is_rejected():
    with pytest.raises(NotImplementedError, match="bimamba=True"):
        _small_model(bimamba=False)


def test_build_videomamba_namespace_with_pretrained(tmp_path):
    ref = _small_model()
    path = tmp_path / "mini_ckpt.pt"
    torch.save(ref.state_dict(), path)
    model = video_mamba.build_videomamba(_cfg(pretrained=str(path)))
    assert isinstance(model, PretrainVideoMamba)
    for k, v in ref.state_dict().items():
        torch.testing.assert_close(model.state_dict()[k], v)


def test_load_state_dict_rejects_wrapped_checkpoint(tmp_path):
    path = tmp_path / "wrapped.pt"
    torch.save({"model": _small_model().state_dict()}, path)
    with pytest.raises(ValueError, match="plain state_dict checkpoint"):
        video_mamba.build_videomamba(_cfg(pretrained=str(path)))


def test_build_videomamba_requires_channels_attr(tmp_path):
    cfg = _cfg()
    del cfg.vision_encoder.channels
    cfg.vision_encoder.in_chans = 3
    with pytest.raises(AttributeError):
        video_mamba.build_videomamba(cfg)


def test_load_state_dict_uses_weights_only(tmp_path, monkeypatch):
    model = _small_model()
    path = tmp_path / "mini_ckpt.pt"
    torch.save(model.state_dict(), path)
    seen = {}
    orig = vm_module.torch.load

    def wrapped(*a, **kw):
        seen.update(kw)
        return orig(*a, **kw)

    monkeypatch.setattr(vm_module.torch, "load", wrapped)
    load_state_dict(str(path), model, ckpt_num_frame=4, num_frames=4)
    assert seen.get("weights_only") is True


def test_load_state_dict_interpolates_pos_embed_for_non_square_target(tmp_path):
    src = _small_model(img_size=8, patch_size=4)
    dst = _small_model(img_size=(8, 12), patch_size=4)
    path = tmp_path / "src.pt"
    torch.save(src.state_dict(), path)
    load_state_dict(str(path), dst, ckpt_num_frame=4, num_frames=4)
    assert dst.pos_embed.shape == (1, 1 + (8 // 4) * (12 // 4), 16)


def test_load_state_dict_interpolates_temporal_embedding(tmp_path):
    src = _small_model(num_frames=4)
    dst = _small_model(num_frames=8)
    path = tmp_path / "src.pt"
    torch.save(src.state_dict(), path)
    load_state_dict(str(path), dst, ckpt_num_frame=4, num_frames=8)
    assert dst.temporal_pos_embedding.shape == (1, 8, 16)
    with pytest.raises(ValueError, match="ckpt_num_frame must be a positive integer"):
        load_state_dict(str(path), dst, ckpt_num_frame=0, num_frames=8)


def test_no_weight_decay_and_num_layers():
    model = _small_model()
    assert "temporal_pos_embedding" in model.no_weight_decay()
    assert model.get_num_layers() == 2


def test_state_dict_keys_match_reference_layout():
    m = _small_model(fused_add_norm=True, rms_norm=True, residual_in_fp32=True)
    keys = set(m.state_dict())
    expect = {"cls_token", "pos_embed", "temporal_pos_embedding", "patch_embed.proj.weight",
              "patch_embed.proj.bias", "norm.weight", "pool_norm.weight", "pool_norm.bias"}
    for i in range(2):
        for k in ("A_log", "D", "in_proj.weight", "conv1d.weight", "conv1d.bias",
                  "x_proj.weight", "dt_proj.weight", "dt_proj.bias", "out_proj.weight"):
            expect.add(f"layers.{i}.mixer.{k}")
        expect.add(f"layers.{i}.norm.weight")
    assert keys == expect


def test_param_counts_match_survey():
    ti = PretrainVideoMamba(depth=24, embed_dim=192, num_frames=8)
    assert sum(p.numel() for p in ti.parameters()) == 6_228_864


# ------------------------------------------------------------------ device guard
def test_mamba_forward_requires_cuda_tensor_inputs():
    model = Mamba(d_model=8, d_state=4, d_conv=2, expand=2, use_fast_path=False,
                  layer_idx=0).eval()
    with pytest.raises(RuntimeError, match="requires CUDA tensors"):
        model(torch.randn(1, 2, 8))


def test_encoder_forward_requires_cuda_tensor_inputs():
    model = _small_model().eval()
    with pytest.raises(RuntimeError, match="requires CUDA tensors"):
        model(torch.randn(1, 3, 4, 8, 8))


def test_tubelet_validation_happens_before_compute():
    model = _small_model(kernel_size=2, num_frames=8)
    x = torch.randn(1, 3, 5, 8, 8)
    with pytest.raises(ValueError, match="must be divisible by tubelet size"):
        model(x, mask=None, use_image=False)
    with pytest.raises(ValueError, match="must be divisible by tubelet size"):
        model.forward_features(x, mask=None, use_image=False)
    with pytest.raises(ValueError, match="x must have shape"):
        model(torch.randn(3, 4, 8, 8))


def test_block_and_refiner_construct():
    b = create_block(16, ssm_cfg={"use_fast_path": False}, rms_norm=False, fused_add_norm=False,
                     residual_in_fp32=False, layer_idx=0)
    assert b.layer_idx == 0 and b.mixer.bimamba is False
    r = video_mamba.BiMambaRefinerBlock(16, layer_idx=3)
    assert r.block_bwd.layer_idx == 1_000_003
    fs, bs = r.allocate_state(2)
    assert fs[0].shape == (2, 32, 4) and bs[1].shape == (2, 32, 16)


def test_rectangular_patch_size_builds_the_reference_conv():
    # the reference's PatchEmbed takes patch_size as (ph, pw) (videomamba.py:340-364)
    m = video_mamba.PretrainVideoMamba(img_size=16, patch_size=(8, 4), depth=1, embed_dim=16,
                                       num_frames=4)
    pe = m.patch_embed
    assert pe.patch_size == (8, 4) and pe.num_patches == 2 * 4
    assert pe.proj.weight.shape == (16, 3, 1, 8, 4) and pe.proj.stride == (1, 8, 4)
    assert m.pos_embed.shape == (1, 1 + 8, 16)
    assert m._spatial_token_grid(16, 16) == (2, 4)


# ------------------------------------------------------------------ C ABI
def test_library_loads_and_exports_every_header_symbol():
    lib = _lib.load()
    assert lib.vm_abi_version() == _lib.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "videomamba_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|long long|const char\*)\s+(vm_\w+)\(", header, re.M))
    assert declared == set(_lib.EXPORTED)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    # the types too: every prototype against the hand-written ctypes table, argument by
    # argument.  A declarator this parser does not know fails (KeyError), it is not skipped.
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    code = re.sub(r"//[^\n]*", " ", code)
    code = "\n".join(ln for ln in code.splitlines() if not ln.lstrip().startswith("#"))
    scalars = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float,
               "vm_stream_t": ctypes.c_void_p}
    returns = {**scalars, "const char*": ctypes.c_char_p}

    def ctype(decl):  # "const float* A" -> c_void_p, "long long u_sb" -> c_longlong
        m = re.fullmatch(r"(?:const\s+)?(\w+(?:\s+\w+)*?)\s*(\*?)\s*(\w+)", " ".join(decl.split()))
        assert m, f"unparsed declarator {decl!r}"
        return ctypes.c_void_p if m.group(2) else scalars[m.group(1)]

    protos = re.findall(r"([\w ]+?\*?)\s*\b(vm_\w+)\s*\(([^)]*)\)\s*;", code)
    parsed = {}
    for ret, name, params in protos:
        params = params.strip()
        args = [] if params in ("", "void") else [ctype(p) for p in params.split(",")]
        parsed[name] = (args, returns[" ".join(ret.split())])
    assert len(parsed) == len(protos) == 43 and set(parsed) == declared
    assert "vm_" not in re.sub(r"\bvm_\w+\s*\([^)]*\)\s*;|\bvm_stream_t\b", "", code), \
        "a vm_ declaration the prototype pattern did not take"
    for name, want in parsed.items():
        assert (list(_lib._SIGNATURES[name][0]), _lib._SIGNATURES[name][1]) == want, name


def test_abi_rejects_bad_arguments_without_gpu():
    lib = _lib.load()
    rc = lib.vm_selective_scan_fwd(*([None, 0, 0, 0] * 2), None, *([None, 0, 0, 0] * 2),
                                   None, None, 0, 0, 0, None, 0, None, 0, 0, 0, None, 0, 0, 0,
                                   None, 0, 0, 0, 0, 1, 1, 1, 16, 0, 0, None, 0, None, 0, None)
    assert rc == -1
    assert b"null required pointer" in lib.vm_last_error()
    rc = lib.vm_add_norm_fwd(None, 0, None, 0, None, None, None, 0, None, 0, 1, 8, 1e-5, 1, None)
    assert rc == -1


def test_scan_workspace_query_without_gpu():
    lib = _lib.load()
    # small batch, long sequence: the segmented token-major form wants scratch
    assert lib.vm_selective_scan_workspace_bytes(1, 1152, 3137, 16, 0) > 0
    # a chip-filling batch (>= 1.25 waves per SIMD of 64-channel groups) runs single-pass
    assert lib.vm_selective_scan_workspace_bytes(72, 1152, 3137, 16, 0) == 0
    assert lib.vm_selective_scan_workspace_bytes(1, 1152, 3137, 17, 0) == 0
    # an explicit segment request (the ABI's only configuration argument) is honoured
    one = lib.vm_selective_scan_workspace_bytes(2, 64, 100, 16, 1)
    four = lib.vm_selective_scan_workspace_bytes(2, 64, 100, 16, 4)
    # max of the chunked form (one 8-segment block: 9 x 64 x 17 floats per batch row) and
    # the legacy summary / carry / final form (4 x 64 x 33 floats per batch row)
    chunked = 2 * (9 * 64 * 17) * 4
    legacy = 2 * 4 * 64 * (2 * 16 + 1) * 4
    assert one == 0 and four == max(chunked, legacy)
    # the one-launch form's sync buffer: a 16-byte header (error word, epoch, start count),
    # then a {tag, value} granule per (row, 64-channel group, block, 16 states + delta sum,
    # channel)
    assert lib.vm_selective_scan_sync_bytes(2, 64, 100, 16, 4) == 16 + 2 * 1 * 1 * 17 * 64 * 8
    assert lib.vm_selective_scan_sync_bytes(72, 1152, 3137, 16, 0) == 0
    assert lib.vm_selective_scan_sync_bytes(1, 1152, 3137, 16, 0) > 0


def test_scan_segment_cost_model_choices_without_gpu():
    """The measured segment cost model (vm_scan_plan.h::choose_segments, fitted to
    profiles/r02_scan_segments_sweep.jsonl) as seen through the sync-buffer query:
    nblk blocks of {tag, value} granules per (row, 64-channel group) at M-16f (D = 1152, 18
    groups).  B = 1:
    S = 112 -> 14 blocks of 8 segments (252 workgroups, one per CU); B = 2 .. 8: S = 56 ->
    7 blocks (the round-1 wave-target rule chose 2-3x slower counts there); B >= 72 (1,280+
    waves): single pass, no segments."""
    lib = _lib.load()
    nblk = lambda B, L: (lib.vm_selective_scan_sync_bytes(B, 1152, L, 16, 0) - 16) // (B * 18 * 17 * 64 * 8)  # noqa: E731
    assert nblk(1, 3137) == 14 and nblk(1, 12545) == 14
    assert nblk(2, 3137) == nblk(4, 3137) == nblk(8, 3137) == 7
    assert lib.vm_selective_scan_sync_bytes(72, 1152, 3137, 16, 0) == 0


def _scan_size_query_rows():
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "scan_size_queries.json")))
    assert table["columns"] == ["batch", "dim", "seqlen", "segments", "dstate", "workspace_bytes",
                                "sync_bytes", "chunk_steps"]
    return table["rows"]


def test_scan_size_queries_reproduce_the_recorded_table():
    """The three size queries against tests/golden/scan_size_queries.json: their values as
    recorded from the library built at the commit the file names (before the host side was
    folded into vm_scan_plan.h::plan_scan), without a device, so with the 256-CU
    calibration.  Every row must come back unchanged."""
    lib = _lib.load()
    rows = _scan_size_query_rows()
    assert len(rows) >= 300
    bad = []
    for b, d, l, seg, n, ws, sync, steps in rows:
        got = (lib.vm_selective_scan_workspace_bytes(b, d, l, n, seg),
               lib.vm_selective_scan_sync_bytes(b, d, l, n, seg),
               lib.vm_selective_scan_chunk_steps(b, d, l, n, seg))
        if got != (ws, sync, steps):
            bad.append(((b, d, l, seg, n), (ws, sync, steps), got))
    assert not bad, bad[:5]


def test_scan_dtproj_segmented_pays_counts_the_library_s_workgroups():
    """kernels.scan_dtproj_segmented_pays asks the library for the chunked scan's workgroup
    count (vm_selective_scan_dtproj_fits; plan_scan's one-launch test counts the same grid).
    For every segmented row of the recorded table that count must equal the one read off the
    sync-buffer size (one 17 x 64 granule block of 8 bytes per workgroup after the 16-byte
    header): with exactly that many CUs a segment of at most 64 steps pays, with one fewer it
    does not."""
    from videomamba_amd.kernels import scan_dtproj_segmented_pays as pays
    seen = 0
    for b, d, l, seg, n, ws, sync, steps in _scan_size_query_rows():
        if steps <= 0:
            continue
        wgs, rem = divmod(sync - 16, 17 * 64 * 8)
        assert rem == 0 and wgs >= 1
        if n != 16:  # dt_proj inside the scan takes 16 states only (the mixer's gate asked too)
            assert not pays(b, d, l, n, segments=seg, cus=wgs), (b, d, l, seg)
            continue
        assert pays(b, d, l, n, segments=seg, cus=wgs) == (steps <= 64), (b, d, l, seg)
        if wgs > 1:  # cus=0 asks for the current device
            assert not pays(b, d, l, n, segments=seg, cus=wgs - 1), (b, d, l, seg)
        seen += steps <= 64
    assert seen >= 100


def test_scan_plan_check_program_passes_under_sanitizers(tmp_path):
    """tests/host/scan_plan_check.cpp walks vm_scan_plan.h::plan_scan over shapes x CU
    counts x operand facts x buffer offers and exits non-zero on any inconsistent plan
    (overlapping workspace regions, uncovered steps, a one-launch grid that is not resident,
    ...).  Built as a program of its own with the host compiler under ASan + UBSan, the
    sanitizer runtimes linked into the program (clang's default; g++ needs the flags)."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"
    cxx = [rocm_clang] if os.path.exists(rocm_clang) else \
        [shutil.which("g++") or "g++", "-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "scan_plan_check")
    subprocess.run(cxx + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "videomamba_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "scan_plan_check.cpp"), "-o", exe],
                   check=True, timeout=120)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout


def test_library_reads_no_environment():
    """The C library has no configuration channel besides its arguments:
    no getenv in any product source."""
    csrc = os.path.join(ROOT, "videomamba_amd", "csrc")
    for name in os.listdir(csrc):
        if name.endswith((".hip", ".h")):
            assert "getenv" not in open(os.path.join(csrc, name)).read(), name


def test_options_override_and_validation():
    from videomamba_amd import options
    assert options.get().mixer_layout == "auto" and options.get().scan_segments == 0
    with options.override(mixer_layout="tm", scan_segments=8) as o:
        assert options.get() is o and o.scan_segments == 8
    assert options.get().mixer_layout == "auto"
    with pytest.raises(ValueError):
        with options.override(mixer_layout="xx"):
            pass


def test_scan_sync_error_word_is_reported_on_the_host():
    """The one-launch scan's bounded hand-off (vm_scan_seq.hip, PASS 3): a block whose wait
    runs out sets word 0 of the sync buffer (and writes NaN outputs).  The host-side check
    reads that word from a host copy — no GPU involved: a clean header is 0, a set word is
    1, a short buffer is rejected, and check paths raise."""
    from videomamba_amd import kernels as K
    lib = _lib.load()
    nbytes = lib.vm_selective_scan_sync_bytes(1, 1152, 3137, 16, 0)
    buf = torch.zeros(nbytes, dtype=torch.uint8)
    assert K.scan_sync_status(buf) == 0
    buf.view(torch.int32)[0] = 1  # what a timed-out block stores
    assert K.scan_sync_status(buf) == 1
    buf.view(torch.int32)[0] = 0
    buf[4:] = 7  # epoch, start count and granules do not count as errors
    assert K.scan_sync_status(buf) == 0
    assert lib.vm_selective_scan_sync_status(buf.data_ptr(), 8) == -1
    assert b"sync header" in lib.vm_last_error()


@pytest.mark.parametrize("embed_dim,depth", [(192, 24), (384, 24), (576, 32)])
@pytest.mark.parametrize("frames", [8, 16])
def test_graph_workspace_covers_first_and_continuation_chunks(embed_dim, depth, frames):
    """StreamingChunkGraph's scratch must fit both chunk kinds: the first chunk scans
    L = T*196 + 1 tokens, continuation chunks L - 1, and the segment cost model may choose
    more segments (more scratch) for L - 1 (Ti-16f at B = 1 needed 11.35 MB for
    L - 1 against 10.14 MB sized for L).  Ti / S / M at 224 px, B = 1 .. 8."""
    from videomamba_amd import kernels as K
    from videomamba_amd.graphs import chunk_workspace_bytes
    m = PretrainVideoMamba(depth=depth, embed_dim=embed_dim, num_frames=frames)
    mx = next(iter(m._mixers()))
    short_wins = 0
    for B in range(1, 9):
        need, sync_need = chunk_workspace_bytes(m, B, frames, 14, 14)
        for L in (frames * 196 + 1, frames * 196):
            assert need >= K.scan_workspace_bytes(B, mx.d_inner, L, mx.d_state), (B, L)
            assert sync_need >= K.scan_sync_bytes(B, mx.d_inner, L, mx.d_state), (B, L)
        L = frames * 196 + 1
        short_wins += (K.scan_workspace_bytes(B, mx.d_inner, L - 1, mx.d_state)
                       > K.scan_workspace_bytes(B, mx.d_inner, L, mx.d_state))
    if (embed_dim, frames) == (192, 16):
        assert short_wins > 0  # the case the first-chunk-only sizing missed


def test_conv_proj_wide_offset_limit_is_rejected_on_the_host():
    """The wide conv_proj kernel (batch > 8) addresses x rows, the conv state and u rows
    through buffer resources with 31-bit offsets; vm_conv_proj_fwd rejects shapes past them
    before any HIP call (pointers here are never dereferenced): a 300k-token sequence of
    xz at D = 1152 is past the limit."""
    lib = _lib.load()
    D, E, Ep, R = 1152, 68, 80, 36
    fake = lambda i: ctypes.c_void_p((i + 1) << 20)  # noqa: E731  16-byte aligned, unused

    def call(L, batch):
        Lp = L
        return lib.vm_conv_proj_fwd(
            fake(0), Lp * 2 * D, 2 * D, fake(1), fake(2),
            None, 0, 0, 0, None, 0, 0, 0,
            fake(3), E, Ep, None, R, 0,
            fake(4), Lp * D, D, fake(5), Lp * E, E, None, 0, 0,
            None, 0, Lp, batch, D, L, 4, _lib.VM_DTYPE_BF16, None, 0, None)

    assert call(300_000, 9) == -1
    assert b"31-bit" in lib.vm_last_error()
    assert call(300_000, 0) == 0  # empty batch: nothing to launch, nothing to check


def _conv_proj_query_rows():
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "conv_proj_queries.json")))
    assert table["columns"] == [
        "batch", "out_len", "seqlen", "dim", "e", "e_pad", "r_pad", "k", "cs_dtype",
        "dt_softplus", "has_dt", "width", "fits", "workspace_bytes", "in_proj_fits",
        "in_proj_workspace_bytes", "cm_workspace_bytes"]
    return table["rows"]


def test_conv_proj_queries_reproduce_the_recorded_table():
    """The five host queries of the mixer middle against tests/golden/conv_proj_queries.json:
    their answers as recorded from the library built at the commit the file names (before
    the host side was folded into vm_conv_proj_plan.h::plan_conv_proj), over shapes on both
    sides of every form limit.  The strides are the mixer's (see gen_conv_proj_queries.py).
    Every row must come back unchanged."""
    lib = _lib.load()
    rows = _conv_proj_query_rows()
    assert len(rows) >= 300
    bad = []
    for row in rows:
        b, lp, l, d, e, ep, rp, k, cs, spd, has_dt, w = row[:12]
        got = [lib.vm_conv_proj_fits(b, lp, l, d, e, rp, spd, lp * 2 * d, 2 * d, int(cs >= 0),
                                     max(cs, 0), d * w, w, w, d),
               lib.vm_conv_proj_workspace_bytes(b, lp, d, e),
               lib.vm_in_proj_conv_proj_fits(k, b, lp, d, e, ep, rp, w, has_dt),
               lib.vm_in_proj_conv_proj_workspace_bytes(b, lp, d, e),
               lib.vm_conv_proj_cm_workspace_bytes(b, lp, d, e)]
        if got != row[12:]:
            bad.append((row[:12], row[12:], got))
    assert not bad, bad[:5]


def test_conv_proj_plan_check_program_passes_under_sanitizers(tmp_path):
    """tests/host/conv_proj_plan_check.cpp walks vm_conv_proj_plan.h::plan_conv_proj over
    shapes x options x the three entries and exits non-zero on any plan whose form differs
    from the rules written out there, whose template selectors are not instantiated, whose
    tiles do not cover the tokens, whose workspace is below what its kernels index, whose
    buffer-resource extents reach 2^31 bytes or whose LDS does not fit.  Built as a program
    of its own under ASan + UBSan, as scan_plan_check.cpp is."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"
    cxx = [rocm_clang] if os.path.exists(rocm_clang) else \
        [shutil.which("g++") or "g++", "-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "conv_proj_plan_check")
    subprocess.run(cxx + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "videomamba_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "conv_proj_plan_check.cpp"), "-o", exe],
                   check=True, timeout=120)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout


def test_conv_proj_small_max_batch_matches_the_library():
    """kernels.CONV_PROJ_SMALL_MAX_BATCH is the library's kSkMaxBatch: the workspace query
    answers up to that batch and reports 0 one above."""
    from videomamba_amd import kernels as K
    lib = _lib.load()
    B = K.CONV_PROJ_SMALL_MAX_BATCH
    assert lib.vm_conv_proj_workspace_bytes(B, 3144, 1152, 68) > 0
    assert lib.vm_conv_proj_workspace_bytes(B + 1, 3144, 1152, 68) == 0


def _fake(i, off=0):
    return ctypes.c_void_p(((i + 1) << 20) + off)  # 16-byte aligned (off 0), never dereferenced


def _conv_proj_tm_call(lib, **over):
    """vm_conv_proj_fwd on fake pointers at the mixer's M geometry; `over` replaces
    arguments by name."""
    a = dict(D=1152, E=68, Ep=80, R=36, Rp=64, L=3137, Lp=3144, batch=2, width=4,
             dtype=_lib.VM_DTYPE_BF16, spd=0, xz=_fake(0), cw=_fake(1), cs_in=None, cs_out=None,
             wx=_fake(3), wdt=_fake(4), u=_fake(5), xdbl=_fake(6), dt=_fake(7), ws=_fake(8),
             ws_bytes=1 << 40, u_sb=None, xz_sb=None)
    a.update(over)
    s = SimpleNamespace(**a)
    u_sb = s.Lp * s.D if s.u_sb is None else s.u_sb
    xz_sb = s.Lp * 2 * s.D if s.xz_sb is None else s.xz_sb
    return lib.vm_conv_proj_fwd(
        s.xz, xz_sb, 2 * s.D, s.cw, _fake(2),
        s.cs_in, 0, s.D * 4, 4, s.cs_out, 0, s.D * 4, 4,
        s.wx, s.E, s.Ep, s.wdt, s.R, s.Rp,
        s.u, u_sb, s.D, s.xdbl, s.Lp * s.E, s.E, s.dt, s.Lp * s.D, s.D,
        None, s.spd, s.Lp, s.batch, s.D, s.L, s.width, s.dtype, s.ws, s.ws_bytes, None)


def _in_proj_conv_proj_call(lib, **over):
    a = dict(D=1152, K=576, E=68, Ep=80, R=36, Rp=64, L=3137, Lp=3144, batch=2, width=4,
             hn=_fake(0), w_in=_fake(1), z=_fake(2), cw=_fake(3), cs_in=None, cs_out=None,
             wx=_fake(5), wdt=_fake(6), u=_fake(7), xdbl=_fake(8), dt=_fake(9), ws=_fake(10),
             ws_bytes=1 << 40, ldh=None)
    a.update(over)
    s = SimpleNamespace(**a)
    return lib.vm_in_proj_conv_proj_fwd(
        s.hn, s.K if s.ldh is None else s.ldh, s.w_in, s.K, s.K, s.z, s.D, s.cw, _fake(4),
        s.cs_in, 0, s.D * 4, 4, s.cs_out, 0, s.D * 4, 4,
        s.wx, s.E, s.Ep, s.wdt, s.R, s.Rp,
        s.u, s.D, s.xdbl, s.E, s.dt, s.D,
        s.Lp, s.batch, s.D, s.L, s.width, s.ws, s.ws_bytes, None)


def _conv_proj_cm_call(lib, **over):
    a = dict(D=1152, E=68, Ep=80, R=36, Rp=64, L=3137, Lp=3144, batch=2, width=4,
             xz=_fake(0), cw=_fake(1), cs_in=None, cs_out=None, wx=_fake(3), wdt=_fake(4),
             u=_fake(5), xdbl=_fake(6), dt=_fake(7), ws=_fake(8), ws_bytes=1 << 40, x_sd=None)
    a.update(over)
    s = SimpleNamespace(**a)
    ntok = s.batch * s.Lp
    return lib.vm_conv_proj_cm_fwd(
        s.xz, ntok if s.x_sd is None else s.x_sd, s.cw, _fake(2),
        s.cs_in, 0, s.D * 4, 4, s.cs_out, 0, s.D * 4, 4,
        s.wx, s.E, s.Ep, s.wdt, s.R, s.Rp,
        s.u, ntok, s.xdbl, ntok, s.dt, ntok,
        s.Lp, s.batch, s.D, s.L, s.width, s.ws, s.ws_bytes, None)


# 9 splits x (2 x 3144) tokens x 68 floats: the token-major partials of the calls above;
# the channel-major layout [split][e][tok] has the same size at E % 4 == 0
_SK_NEED = 9 * 2 * 3144 * 68 * 4

# (entry, replaced arguments, return code, distinguishing part of vm_last_error()), every
# row as the library at 194923f (before vm_conv_proj_plan.h) answered it.  Refused calls and
# empty batches only: an accepted call would launch on the fake pointers.
_CONV_PROJ_REFUSALS = [
    # null pointer
    (_conv_proj_tm_call, dict(xz=None), -1, b"vm_conv_proj_fwd: null required pointer"),
    (_conv_proj_tm_call, dict(wdt=None), -1, b"vm_conv_proj_fwd: null required pointer"),
    (_in_proj_conv_proj_call, dict(hn=None), -1, b"vm_in_proj_conv_proj_fwd: null required pointer"),
    (_in_proj_conv_proj_call, dict(z=None), -1, b"vm_in_proj_conv_proj_fwd: null required pointer"),
    (_conv_proj_cm_call, dict(dt=None), -1, b"vm_conv_proj_cm_fwd: null required pointer"),
    # shape
    (_conv_proj_tm_call, dict(D=1100), -1, b"vm_conv_proj_fwd: unsupported shape (bf16, dim % 64"),
    (_conv_proj_tm_call, dict(Ep=144, E=130), -1, b"vm_conv_proj_fwd: unsupported shape"),
    (_conv_proj_tm_call, dict(Rp=96), -1, b"vm_conv_proj_fwd: unsupported shape"),
    (_conv_proj_tm_call, dict(dtype=_lib.VM_DTYPE_F32), -1, b"vm_conv_proj_fwd: unsupported shape"),
    (_in_proj_conv_proj_call, dict(K=1024), -1,
     b"vm_in_proj_conv_proj_fwd: unsupported shape (bf16; k in {192 .. 1536} by 64-steps; "
     b"batch <= 8, out_len >= 56 and even, dim % 128 == 0 and <= 2048, R + 2N <= 76, "
     b"e_pad <= 80"),
    (_in_proj_conv_proj_call, dict(batch=9), -1, b"vm_in_proj_conv_proj_fwd: unsupported shape"),
    (_in_proj_conv_proj_call, dict(batch=0), -1, b"vm_in_proj_conv_proj_fwd: unsupported shape"),
    (_in_proj_conv_proj_call, dict(Lp=54, L=50), -1, b"vm_in_proj_conv_proj_fwd: unsupported shape"),
    (_in_proj_conv_proj_call, dict(D=2176), -1, b"vm_in_proj_conv_proj_fwd: unsupported shape"),
    (_in_proj_conv_proj_call, dict(D=1088), -1, b"vm_in_proj_conv_proj_fwd: unsupported shape"),
    (_in_proj_conv_proj_call, dict(E=78), -1, b"vm_in_proj_conv_proj_fwd: unsupported shape"),
    (_in_proj_conv_proj_call, dict(Ep=96), -1, b"vm_in_proj_conv_proj_fwd: unsupported shape"),
    (_in_proj_conv_proj_call, dict(Rp=96), -1, b"vm_in_proj_conv_proj_fwd: unsupported shape"),
    (_conv_proj_cm_call, dict(Lp=3140), -1, b"vm_conv_proj_cm_fwd: unsupported shape (dim % 64"),
    (_conv_proj_cm_call, dict(D=1100), -1, b"vm_conv_proj_cm_fwd: unsupported shape"),
    # alignment
    (_conv_proj_tm_call, dict(xz=_fake(0, 2)), -1, b"vm_conv_proj_fwd: xz / u / dt / weights need 16-byte"),
    (_conv_proj_tm_call, dict(Lp=3145), -1, b"vm_conv_proj_fwd: xz / u / dt / weights need 16-byte"),
    (_conv_proj_tm_call, dict(D=8256), -1, b"x_dbl 4-byte aligned, even out_len and e, dim <= 8192"),
    (_in_proj_conv_proj_call, dict(hn=_fake(0, 2)), -1, b"16-byte aligned rows; hn under 2 GB"),
    (_in_proj_conv_proj_call, dict(ldh=580), -1, b"vm_in_proj_conv_proj_fwd: unsupported shape"),
    (_conv_proj_cm_call, dict(u=_fake(5, 8)), -1,
     b"vm_conv_proj_cm_fwd: x / u / dt rows and the weights must be 16-byte aligned"),
    (_conv_proj_cm_call, dict(x_sd=2 * 3144 + 4), -1, b"must be 16-byte aligned"),
    # batch-contiguity (token-major outputs)
    (_conv_proj_tm_call, dict(u_sb=3144 * 1152 + 8), -1,
     b"vm_conv_proj_fwd: u / x_dbl / dt must be batch-contiguous (sb == out_len * sl)"),
    # aliasing
    (_conv_proj_tm_call, dict(cs_in=_fake(9), cs_out=_fake(9)), -1,
     b"vm_conv_proj_fwd: conv_state_out must not alias conv_state_in"),
    (_in_proj_conv_proj_call, dict(cs_in=_fake(11), cs_out=_fake(11)), -1,
     b"vm_in_proj_conv_proj_fwd: conv_state_out must not alias conv_state_in"),
    (_conv_proj_cm_call, dict(cs_in=_fake(9), cs_out=_fake(9)), -1,
     b"vm_conv_proj_cm_fwd: conv_state_out must not alias conv_state_in"),
    # missing or short workspace
    (_conv_proj_tm_call, dict(ws=None), -1,
     b"vm_conv_proj_fwd: batch <= 8 needs a workspace of %d bytes (vm_conv_proj_workspace_bytes)" % _SK_NEED),
    (_conv_proj_tm_call, dict(ws_bytes=_SK_NEED - 1), -1, b"needs a workspace of %d bytes" % _SK_NEED),
    # the fused form writes no partials, yet the entry asks for them at every small batch
    (_conv_proj_tm_call, dict(ws_bytes=0, batch=1), -1, b"needs a workspace of %d bytes" % (_SK_NEED // 2)),
    (_in_proj_conv_proj_call, dict(ws=None), -1,
     b"vm_in_proj_conv_proj_fwd: needs a workspace of %d bytes "
     b"(vm_in_proj_conv_proj_workspace_bytes)" % _SK_NEED),
    (_in_proj_conv_proj_call, dict(ws_bytes=_SK_NEED - 1), -1, b"needs a workspace of %d bytes" % _SK_NEED),
    (_conv_proj_cm_call, dict(ws=None), -1,
     b"vm_conv_proj_cm_fwd: workspace of %d bytes required" % _SK_NEED),
    (_conv_proj_cm_call, dict(ws_bytes=_SK_NEED - 1), -1, b"workspace of %d bytes required" % _SK_NEED),
    # 31-bit offsets
    (_conv_proj_tm_call, dict(batch=9, L=300_000, Lp=300_000), -1,
     b"vm_conv_proj_fwd: batch > 8 needs a sequence of xz under 1 GiB (31-bit buffer offsets)"),
    (_conv_proj_tm_call, dict(batch=2, spd=1, L=300_000, Lp=300_000), -1, b"31-bit buffer offsets"),
    (_in_proj_conv_proj_call, dict(batch=8, L=300_000, Lp=300_000), -1, b"hn under 2 GB"),
    # empty batch: nothing to launch (the in_proj entry refuses it, above)
    (_conv_proj_tm_call, dict(batch=0), 0, None),
    (_conv_proj_tm_call, dict(batch=0, ws=None), 0, None),
    (_conv_proj_cm_call, dict(batch=0), 0, None),
    (_conv_proj_cm_call, dict(batch=0, ws=None), 0, None),
    # batch-contiguity of xz: the small forms address x as one run of token rows (kept last:
    # the rows above keep the indices they were recorded under)
    (_conv_proj_tm_call, dict(xz_sb=(3144 + 8) * 2 * 1152), -1,
     b"vm_conv_proj_fwd: the small-batch forms need batch-contiguous xz rows "
     b"(xz_sb == out_len * xz_sl), got xz_sb %d" % ((3144 + 8) * 2 * 1152)),
]


@pytest.mark.parametrize("row", range(len(_CONV_PROJ_REFUSALS)))
def test_conv_proj_entries_refuse_as_recorded(row):
    """The three mixer-middle entries refuse on the host, before any HIP call, with the
    return code and message they had before the plan (fake pointers, never dereferenced):
    null pointer, shape, alignment, batch-contiguity, aliasing, workspace, 31-bit offsets.
    The gapped-xz row is the one refusal added since: a small form with batch > 1 and
    xz_sb != out_len * xz_sl."""
    call, over, rc, text = _CONV_PROJ_REFUSALS[row]
    lib = _lib.load()
    assert call(lib, **over) == rc
    if text is not None:
        assert text in lib.vm_last_error(), lib.vm_last_error()


def test_conv_proj_fits_query_routes_long_sequences_to_the_unfused_path():
    """the wide conv_proj form's 31-bit offsets reject ~230k-token sequences at
    batch > 8; vm_conv_proj_fits reports that on the host and the mixer's fused-path test
    mirrors it, so such a forward takes the unfused conv + projection path instead of
    raising.  Small batches (split-K / fused forms, 64-bit addressing) always fit."""
    from videomamba_amd import kernels as K
    from videomamba_amd.mamba_simple import Mamba
    D, E = 1152, 68
    fits = lambda B, L: K.conv_proj_fits(B, L, L, D, E, 64, (L * 2 * D, 2 * D), D, None, 4)  # noqa: E731
    assert fits(9, 3144) and fits(448, 3144) and fits(8, 300_000)
    assert not fits(9, 300_000)
    mx = Mamba(d_model=576).to(torch.bfloat16)
    shape_only = lambda B, L: torch.empty(1, 1, 576, dtype=torch.bfloat16).expand(B, L, 576)  # noqa: E731
    assert mx._fused_conv_proj_ok(shape_only(9, 3144), 3137)
    assert not mx._fused_conv_proj_ok(shape_only(9, 300_000), 300_000)
    assert not mx._dtp_ok(shape_only(9, 300_000), 300_000)
    assert mx._fused_conv_proj_ok(shape_only(8, 300_000), 300_000)


def test_linear_rejects_unsupported_k_before_launch():
    """vm_linear_fwd validates k against the unrolled K-step counts it is built
    for and returns VM_E_INVALID (no launch, nothing written) for any other multiple of 64."""
    lib = _lib.load()
    fake = lambda i: ctypes.c_void_p((i + 1) << 20)  # noqa: E731  never dereferenced
    for k in (64, 256, 1024):
        rc = lib.vm_linear_fwd(fake(0), k, fake(1), k, None, fake(2), 64, 128, 64, k,
                               _lib.VM_DTYPE_BF16, None)
        assert rc == -1 and b"k = " in lib.vm_last_error(), k


def _gemm_refusal_table():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_refusals.json")))


def _gemm_refusal_calls():
    """The recorder's own argument marshalling (tests/golden/gen_gemm_refusals.py)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "gen_gemm_refusals", os.path.join(ROOT, "tests", "golden", "gen_gemm_refusals.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_gemm_entries_answer_as_recorded():
    """vm_linear_fwd_form, vm_linear_add_norm_fwd and vm_linear_add_norm_counter_bytes against
    tests/golden/gemm_refusals.json: return code and full vm_last_error() text as recorded
    from the library built at the commit the file names, before the host side was folded into
    vm_gemm_plan.h.  Every call has m <= 0, so none can launch on any device (m == 0 returns
    VM_OK only after the form, shape and K tests; m == -1 is refused by the shape block), and
    the made-up pointers are never dereferenced.  Every row must come back unchanged."""
    lib = _lib.load()
    gen = _gemm_refusal_calls()
    table = _gemm_refusal_table()
    assert table["linear_columns"] == gen.LINEAR_COLUMNS + ["rc", "error"]
    assert table["add_norm_columns"] == gen.ADD_NORM_COLUMNS + ["rc", "error"]
    rows = 0
    bad = []
    for name, call in (("linear_rows", gen.call_linear), ("add_norm_rows", gen.call_add_norm)):
        for row in table[name]:
            assert row[table[name.replace("_rows", "_columns")].index("m")] <= 0
            rc = call(lib, row[:-2])
            got = [rc, "" if rc == 0 else lib.vm_last_error().decode()]
            if got != row[-2:]:
                bad.append((name, row, got))
            rows += 1
    for m, want in table["counter_bytes_rows"]:
        if lib.vm_linear_add_norm_counter_bytes(m) != want:
            bad.append(("counter_bytes", m, want))
        rows += 1
    assert rows >= 150
    assert len(table["counter_bytes_rows"]) >= 12
    assert not bad, bad[:5]


def test_gemm_plan_check_program_passes_under_sanitizers(tmp_path):
    """tests/host/gemm_plan_check.cpp walks vm_gemm_plan.h::plan_linear and
    plan_linear_add_norm over shapes x leading dimensions x forms x alignments x CU counts and
    exits non-zero on any plan whose form differs from the rules written out there, whose
    template selectors are not instantiated, whose grid or tiles do not cover m x n, whose LDS
    does not fit, whose buffer extents reach 2^31 bytes or whose counter bytes are off.  Built
    as a program of its own under ASan + UBSan, as conv_proj_plan_check.cpp is."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"
    cxx = [rocm_clang] if os.path.exists(rocm_clang) else \
        [shutil.which("g++") or "g++", "-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "gemm_plan_check")
    subprocess.run(cxx + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "videomamba_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "gemm_plan_check.cpp"), "-o", exe],
                   check=True, timeout=120)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout


def test_sync_rearm_clears_only_the_error_word():
    """re-arming a sync buffer after a reported timeout zeroes word 0 (the error
    word) only; the epoch (word 1) keeps growing so stale granules of earlier launches never
    carry a later launch's tag."""
    from videomamba_amd import kernels as K
    buf = torch.zeros(64, dtype=torch.uint8)
    words = buf.view(torch.int32)
    words[0], words[1], words[2] = 1, 41, 3
    with pytest.raises(RuntimeError):
        K._SYNC.cache[("cpu", None, 0)] = buf
        try:
            K.check_scan_sync()
        finally:
            del K._SYNC.cache[("cpu", None, 0)]
    assert words[0] == 0 and words[1] == 41 and words[2] == 3


# ------------------------------------------------------------------ the launch layer
def _buffer_kinds():
    from videomamba_amd import kernels as K
    # (cache, override, get, buffers check_* walks | None, fill is zeros, least size,
    #  no bytes gives None, an undersized override raises)
    return {
        "scratch": (K._SCRATCH, K.scratch_override, K.scratch, None, False, 0, True, True),
        "sync": (K._SYNC, K.sync_override, K.sync_buffer, K._SYNC.used, True, 4096, True, False),
        "counters": (K._COUNTERS, K.counter_override, K.counter_buffer, K._COUNTERS.used, True,
                     4096, False, True),
    }


@pytest.mark.parametrize("kind", ["scratch", "sync", "counters"])
def test_buffer_kinds_keep_their_rules(kind):
    """The three per-stream buffer kinds of kernels.py, cell by cell: fill, allocation size,
    what no bytes gives, what an undersized override does, whether overrides are remembered
    for check_*; and what they share: the key, growth by replacement, one buffer per stream."""
    import gc
    cache, override, get, used, zeroed, floor, empty_none, small_raises = _buffer_kinds()[kind]
    cpu = torch.device("cpu")
    s1, s2 = 0xB0F1, 0xB0F2  # made-up streams no other test uses
    try:
        a = get(cpu, s1, 8)
        assert a.dtype == torch.uint8 and a.numel() == max(8, floor)
        assert cache.cache[("cpu", None, s1)] is a and get(cpu, s1, 8) is a
        if zeroed:
            assert not a.any()
        b = get(cpu, s2, 8)  # a second stream, a second buffer
        assert b is not a and cache.cache[("cpu", None, s2)] is b
        big = get(cpu, s1, a.numel() + 64)  # growth replaces the cached buffer
        assert big is not a and big.numel() == a.numel() + 64
        assert cache.cache[("cpu", None, s1)] is big and get(cpu, s1, 8) is big
        if zeroed:
            assert not big.any()
        if empty_none:
            assert get(cpu, s1, 0) is None and get(cpu, s1, -1) is None
        else:
            assert get(cpu, s1, 0) is big
            del cache.cache[("cpu", None, s1)]
            assert get(cpu, s1, 0).numel() == floor
        ov = torch.zeros(32, dtype=torch.uint8)
        with override(ov) as entered:
            assert entered is ov and get(cpu, s1, 32) is ov and get(cpu, s2, 8) is ov
            if small_raises:
                with pytest.raises(RuntimeError, match="_override buffer too small: 32 < 64"):
                    get(cpu, s1, 64)
            else:
                assert get(cpu, s1, 64) is None
            inner = torch.zeros(16, dtype=torch.uint8)
            with override(inner):
                assert get(cpu, s1, 8) is inner
            assert get(cpu, s1, 8) is ov
        assert get(cpu, s2, 8) is b
        if used is None:
            return
        ids = lambda: [id(t) for t in used()]  # noqa: E731
        assert id(ov) in ids() and id(inner) in ids() and id(b) in ids()
        gone = id(ov)
        del ov, entered
        gc.collect()
        assert gone not in ids() and id(inner) in ids()
    finally:
        cache.cache.pop(("cpu", None, s1), None)
        cache.cache.pop(("cpu", None, s2), None)


@pytest.fixture(scope="module")
def launch_gen():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "gen_launch_args", os.path.join(ROOT, "tests", "golden", "gen_launch_args.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_launchers_pass_the_recorded_arguments(launch_gen):
    """Every launcher of kernels.py against tests/golden/launch_args.json, recorded by
    tests/golden/gen_launch_args.py at the commit the table names: the same entry and the same
    argument list, launch by launch, and no entry Python launches left out."""
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "launch_args.json")))
    assert table["commit"] and set(table["cases"]) == {c.__name__ for c in launch_gen.CASES}
    seen, launches = set(), 0
    for case in launch_gen.CASES:
        got = json.loads(json.dumps(launch_gen.run_case(case)))
        want = table["cases"][case.__name__]
        assert [c[0] for c in got] == [c[0] for c in want], case.__name__
        for (entry, a), (_, b) in zip(got, want):
            assert a == b, (case.__name__, entry, [i for i, (p, q) in enumerate(zip(a, b))
                                                   if p != q])
        seen.update(c[0] for c in got)
        launches += len(got)
    assert launches == table["launches"]
    assert seen == launch_gen.launched_entries()
    # with and without the optional tensors: every entry was recorded with some operand once
    # absent (null, or a buffer the launcher allocated itself) and once given by the caller
    kind = lambda p: "null" if p is None else "own" if p == "nonnull" else "given"  # noqa: E731
    for entry in seen:
        rows = [c[1] for calls in table["cases"].values() for c in calls if c[0] == entry]
        ptrs = [i for i, t in enumerate(_lib._SIGNATURES[entry][0][:-1]) if t is ctypes.c_void_p]
        assert any({"given"} < {kind(r[i]) for r in rows} for i in ptrs), entry
