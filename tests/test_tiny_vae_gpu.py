"""LB_GEMM_C64 (csrc/conv3_c64.hip) and the native tiny decoder on a real MI355X.

Kernel: every output element against F.conv2d in float64 with the bounds of tests/_parity.py (derived from the number formats:
K * 2^-24 * |x| . |w| for the fp32 accumulation, 8 fp32 roundings for the epilogue, one fp16 store), inside guard bands and with
NaN-poisoned pads (ldx 72, ldc 68, ldr 76).  The unflagged route of the same library must meet the same bound on the same inputs
(a sanity check on the reference, not a bitwise claim), and the same launch twice must give the same bytes.

Program layer: the replay protocol of tests/_replay.py (recorded; replayed eagerly, in run_range halves, as a hipGraph; parameter
structs destroyed after recording) on a case built here - nothing is appended to its registry.

Decoder: image rel-L2 <= 1e-2, mean |du8| <= 2, >= 99 % of bytes within 4 against the float64 restatement tests/_taesd_ref.py
(the bars of test_vae_tiny_matches_oracle).  The decoder is not pinned against diffusers (not available).
"""
import dataclasses
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import sdxl_ref as R  # noqa: E402  (tiny UNet / VAE configs only)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _replay as RP  # noqa: E402
import _taesd_ref as T  # noqa: E402
from _guard import guarded  # noqa: E402
from _parity import (accumulate_bound, activation_bound, check_elementwise, contraction_bound, epilogue_bound, rnd)  # noqa: E402

DEV = "cuda"
F16, F32, F64 = torch.float16, torch.float32, torch.float64
NAN = float("nan")
LDX, LDC, LDR = 72, 68, 76


def native():
    import latentblending_amd.native as n
    return n


def ops():
    from latentblending_amd.hip import ops as o
    return o


def lib():
    from latentblending_amd.hip import lib as l
    return l


# ====================================================================== kernel, element by element
# name -> (B, stored H, stored W, ups): the smallest shapes at which each mechanism can fail
CASES = {
    "sub_tile_4x4": (1, 4, 4, 0),              # smaller than a tile: a whole-image partial tile
    "ragged_12x20": (2, 12, 20, 0),            # one partial tile row, two tile columns
    "ragged_40x36": (1, 40, 36, 0),            # interior and edge tiles together, ragged both ways
    "ups_6x10": (1, 6, 10, 1),                 # -> 12 x 20: halo parities at a tile seam
    "ups_20x18": (1, 20, 18, 1),               # -> 40 x 36
    "persistent_5x128x128": (5, 128, 128, 0),  # 320 tiles: more than the grid has blocks - the loop, resident weights across samples
}
EPILOGUES = ["plain", "bias_relu", "res_bias_relu", "alpha"]


def _operands(kind, B, H, W, seed):
    """x [B, H, W, 64] fp16 NHWC and w [64, 64, 3, 3] fp16 of one value kind (those of test_value_ranges_gpu.py)."""
    scale = 576 ** -0.5
    if kind == "normal":
        return rnd(B, H, W, 64, seed=seed), rnd(64, 64, 3, 3, seed=seed + 1, scale=scale)
    if kind == "outliers":                      # channel 7 times 64, its weights divided by 8
        x, w = rnd(B, H, W, 64, seed=seed + 2).float(), rnd(64, 64, 3, 3, seed=seed + 3, scale=scale).float()
        x[..., 7] *= 64.0
        w[:, 7] /= 8.0
        return x.half(), w.half()
    if kind == "negative":                      # every product negative: the pre-activation is below zero everywhere
        return rnd(B, H, W, 64, seed=seed + 4).abs() + 0.01, -(rnd(64, 64, 3, 3, seed=seed + 5, scale=scale).abs())
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def conv_case(name, kind="normal"):
    """Operands and the float64 products of one case: computed once, shared by its epilogues, never modified."""
    B, H, W, ups = CASES[name]
    seed = 7000 + 50 * sorted(CASES).index(name)
    x, w = _operands(kind, B, H, W, seed)
    x64 = x.double().permute(0, 3, 1, 2)
    if ups:
        x64 = F.interpolate(x64, scale_factor=2, mode="nearest")
    base = F.conv2d(x64, w.double(), padding=1).permute(0, 2, 3, 1).contiguous()
    ad = F.conv2d(x64.abs(), w.double().abs(), padding=1).permute(0, 2, 3, 1).contiguous()
    bias = rnd(64, seed=seed + 10, dtype=F32)
    if kind == "negative":
        bias = -bias.abs()
    res = rnd(*base.shape, seed=seed + 11)
    return dict(x=x, w=w, bias=bias, res=res, base=base, ad=ad, ups=ups)


def launch(c, epi, flagged, relu_override=None):
    """One launch through lb_gemm_f16 on poisoned / guarded buffers -> (output [B, Ho, Wo, 64] on the CPU, guard checker, raw bits)."""
    o, l = ops(), lib()
    x = c["x"]
    B, H, W, _ = x.shape
    Ho, Wo = H << c["ups"], W << c["ups"]
    xb = torch.full((B * H * W + 64, LDX), NAN, dtype=F16)              # NaN pad columns, NaN rows behind the last pixel
    xb[:B * H * W, :64] = x.reshape(-1, 64)
    xd = xb.to(DEV)[:B * H * W].view(B, H, W, LDX)[..., :64]
    wd = o.pack_conv_weight(c["w"], 64).to(DEV)
    bias = res = None
    alpha = 0.5 if epi == "alpha" else 1.0
    relu = epi in ("bias_relu", "res_bias_relu") if relu_override is None else relu_override
    if epi in ("bias_relu", "res_bias_relu"):
        bias = c["bias"].to(DEV)
    if epi == "res_bias_relu":
        rb = torch.full((B * Ho * Wo + 64, LDR), NAN, dtype=F16)
        rb[:B * Ho * Wo, :64] = c["res"].reshape(-1, 64)
        res = rb.to(DEV)[:B * Ho * Wo].view(B, Ho, Wo, LDR)[..., :64]
    view, chk = guarded(B * Ho * Wo, 64, LDC, F16, DEV)
    out = view.view(B, Ho, Wo, 64)
    flags = (l.GEMM_C64 if flagged else 0) | (l.GEMM_RELU if relu else 0)
    o.gemm(xd, wd, bias=bias, residual=res, flags=flags, alpha=alpha, out=out, splitk_ws=False,
           conv=dict(KH=3, KW=3, stride=1, pad=1, ups=c["ups"]))
    torch.cuda.synchronize()
    return out.cpu(), chk


def reference(c, epi, relu=None):
    """(float64 reference, per-element bound) of one epilogue."""
    alpha = 0.5 if epi == "alpha" else 1.0
    bias = c["bias"] if epi in ("bias_relu", "res_bias_relu") else None
    res = c["res"] if epi == "res_bias_relu" else None
    pre = alpha * c["base"] + (0 if bias is None else bias.double()) + (0 if res is None else res.double())
    relu = epi in ("bias_relu", "res_bias_relu") if relu is None else relu
    if not relu:
        return pre, contraction_bound(None, None, 576, pre, alpha=alpha, bias=bias, residual=res, absdot64=c["ad"])
    pre_bound = accumulate_bound(c["ad"], 576, alpha) + epilogue_bound(pre, bias, res)
    ref = pre.clamp_min(0)
    return ref, activation_bound(pre_bound, ref)


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("name", list(CASES))
def test_c64_conv_elementwise(name, epi, results_log):
    c = conv_case(name)
    ref, bound = reference(c, epi)
    got, chk = launch(c, epi, flagged=True)
    chk.assert_intact(f"c64 {name} {epi}")
    chk.assert_fully_written(f"c64 {name} {epi}")
    check_elementwise(results_log, f"c64_{name}_{epi}", got, ref, bound)
    again, chk2 = launch(c, epi, flagged=True)
    assert torch.equal(chk.bits, chk2.bits), "the same launch twice must give the same bytes"
    plain, chk3 = launch(c, epi, flagged=False)                          # the library's own route: the reference's sanity check
    chk3.assert_intact(f"unflagged {name} {epi}")
    check_elementwise(results_log, f"c64_unflagged_{name}_{epi}", plain, ref, bound)


@pytest.mark.parametrize("name", ["ragged_40x36", "ups_20x18"])
@pytest.mark.parametrize("kind,epi", [("outliers", "plain"), ("outliers", "res_bias_relu"), ("negative", "bias_relu")])
def test_c64_conv_value_kinds(name, kind, epi, results_log):
    """An outlier channel (x 64) and an all-negative pre-activation, whose ReLU output must be exactly zero everywhere."""
    c = conv_case(name, kind)
    ref, bound = reference(c, epi)
    got, chk = launch(c, epi, flagged=True)
    chk.assert_intact(f"c64 {name} {kind}")
    chk.assert_fully_written(f"c64 {name} {kind}")
    check_elementwise(results_log, f"c64_{name}_{kind}_{epi}", got, ref, bound)
    if kind == "negative":
        assert float(ref.abs().max()) == 0.0, "the case must be negative before the ReLU everywhere"
        assert int((got.view(torch.int16) != 0).sum()) == 0, "ReLU of a negative value must store +0 exactly"


EDGE_LO, EDGE_HI = 2048.0, 2390.0      # times the weight 29.297 = 60000 and 70020 (as in test_value_ranges_gpu.py)


@pytest.mark.parametrize("name", ["ragged_40x36", "ups_20x18"])
def test_c64_conv_store_at_the_fp16_edge(name, results_log):
    """Results on both sides of the largest fp16: channel 7's centre tap is +-29.297 (its other taps zero), one image row holds 2048
    there (results +-60000 + O(1): finite, within the bound), another 2390 (+-70020: the infinity of its sign, as .to(float16)
    gives the reference); in between nothing is asserted, and the share of such elements is below 0.5 %."""
    B, H, W, ups = CASES[name]
    x, w = _operands("normal", B, H, W, 7700)
    x, w = x.clone(), w.clone()
    w[:, 7] = 0
    w[:, 7, 1, 1] = (29.297 * (1.0 - 2.0 * (torch.arange(64) % 2))).to(F16)
    x[0, 5, :, 7], x[0, 9, :, 7] = EDGE_LO, EDGE_HI
    x64 = x.double().permute(0, 3, 1, 2)
    if ups:
        x64 = F.interpolate(x64, scale_factor=2, mode="nearest")
    ref = F.conv2d(x64, w.double(), padding=1).permute(0, 2, 3, 1).contiguous()
    ad = F.conv2d(x64.abs(), w.double().abs(), padding=1).permute(0, 2, 3, 1).contiguous()
    c = dict(x=x, w=w, bias=None, res=None, base=ref, ad=ad, ups=ups)
    bound = contraction_bound(None, None, 576, ref, absdot64=ad)
    got = launch(c, "plain", flagged=True)[0].double()
    a = ref.abs()
    below, beyond = a + bound < 65504.0, a - bound >= 65520.0
    share = float((~(below | beyond)).double().mean())
    results_log[f"c64_edge_{name}_between_share"] = share
    assert share < 0.005
    assert int(beyond.sum()) > 0 and int((below & (a > 59000)).sum()) > 0, "the case must reach both sides of the edge"
    assert bool(torch.isfinite(got[below]).all())
    check_elementwise(results_log, f"c64_edge_{name}_below", got[below], ref[below], bound[below])
    want_inf = torch.where(ref[beyond] > 0, torch.full_like(ref[beyond], float("inf")), torch.full_like(ref[beyond], float("-inf")))
    assert torch.equal(got[beyond], want_inf), "results beyond 65520 must store the infinity of their sign"


def test_c64_refuses_on_the_device_what_it_refuses_on_the_host():
    """A flagged problem of another shape is refused before any launch: the guarded output stays untouched."""
    o, l = ops(), lib()
    x = rnd(1, 16, 16, 128, seed=1).to(DEV)
    w = o.pack_conv_weight(rnd(64, 128, 3, 3, seed=2, scale=0.03), 128).to(DEV)
    view, chk = guarded(256, 64, 64, F16, DEV)
    with pytest.raises(RuntimeError, match="LB_GEMM_C64: Cin must be 64"):
        o.gemm(x, w, flags=l.GEMM_C64, out=view.view(1, 16, 16, 64), splitk_ws=False, conv=dict(KH=3, KW=3, stride=1, pad=1))
    torch.cuda.synchronize()
    chk.assert_untouched("refused C64 launch")


# ====================================================================== program layer
def test_c64_recorded_replayed_and_graph_launches_match_a_direct_launch(results_log):
    """Two flagged launches chained (a ReLU conv with bias and residual, then the ups = 1 form reading its output at ldx 72) under
    the whole replay protocol: direct x2, record (nothing written, op names), parameter structs destroyed and every 'same results'
    switch moved, eager replay, the run_range split, hipGraph on two streams, time_ops - all bit for bit, guard bands included."""
    o, l = ops(), lib()
    B, H, W = 2, 12, 20
    c = RP.Case("c64_chain", ["conv3x3_c64", "conv3x3_c64"])
    xb = torch.full((B * H * W + 64, LDX), NAN, dtype=F16)
    xb[:B * H * W, :64] = rnd(B * H * W, 64, seed=8101)
    xd = c.dev(xb)[:B * H * W].view(B, H, W, LDX)[..., :64]
    rb = torch.full((B * H * W + 64, LDR), NAN, dtype=F16)
    rb[:B * H * W, :64] = rnd(B * H * W, 64, seed=8102)
    rd = c.dev(rb)[:B * H * W].view(B, H, W, LDR)[..., :64]
    w1 = c.dev(o.pack_conv_weight(rnd(64, 64, 3, 3, seed=8103, scale=576 ** -0.5), 64))
    w2 = c.dev(o.pack_conv_weight(rnd(64, 64, 3, 3, seed=8104, scale=576 ** -0.5), 64))
    bias = c.dev(rnd(64, seed=8105, dtype=F32))
    mid = c.guarded("mid", B * H * W, 64, LDX, F16).view(B, H, W, 64)
    out = c.guarded("out", B * 2 * H * 2 * W, 64, LDC, F16).view(B, 2 * H, 2 * W, 64)
    RP._decoy(c)

    def thunk():
        o.gemm(xd, w1, bias=bias, residual=rd, flags=l.GEMM_C64 | l.GEMM_RELU, out=mid, splitk_ws=False,
               conv=dict(KH=3, KW=3, stride=1, pad=1))
        o.gemm(mid, w2, flags=l.GEMM_C64, alpha=0.5, out=out, splitk_ws=False, conv=dict(KH=3, KW=3, stride=1, pad=1, ups=1))
    c.thunk = thunk
    rec = RP.run_protocol(c.freeze(), RP.GpuDriver())
    results_log["c64_replay"] = rec
    print("[replay] " + RP.format_record(rec))
    assert rec["eager"] == rec["graph"] == rec["graph_s2"] == rec["time_ops"] == "equal" and rec["ranges"] == "equal(1)"
    assert rec["host_objects"] >= 2


# ====================================================================== decoder
DECODES = [(3, 4), (2, (4, 12)), (1, 8)]


def _latents(B, L, seed=5):
    h, w = (L, L) if isinstance(L, int) else L
    return torch.randn(B, 4, h, w, generator=torch.Generator().manual_seed(seed)).half()


@functools.lru_cache(maxsize=None)
def decoder_reference(B, L):
    """(state dict, latents, float64 image, its uint8 frames): computed once per shape."""
    sd, z = T.synthetic_state_dict(0), _latents(B, L)
    img = T.decode(sd, z)
    return sd, z, img, T.to_u8(img).numpy()


def _bars(log, key, prog, got_u8, img, ref_u8):
    a, b = prog.image_f32[..., :3].permute(0, 3, 1, 2).float().cpu(), img.float()
    r = ((a - b).norm() / (b.norm() + 1e-30)).item()
    d = np.abs(got_u8.astype(np.int32) - ref_u8.astype(np.int32))
    log[key] = {"rel_l2": r, "mean_abs_u8": float(d.mean()), "frac_within_4": float((d <= 4).mean())}
    print(f"[parity] {key}: rel_l2={r:.3e} mean|du8|={d.mean():.3f} within4={(d <= 4).mean():.4f}")
    assert r <= 1e-2 and d.mean() <= 2 and (d <= 4).mean() >= 0.99


@pytest.fixture
def c64_everywhere(monkeypatch):
    """The emitter's rule sets the bit by measured speed, which leaves it off at test sizes: here every 64 -> 64 conv takes it."""
    from latentblending_amd.native import tiny_vae
    monkeypatch.setattr(tiny_vae, "C64_MIN_TILES", 1)


@pytest.mark.parametrize("c64", [True, False])
@pytest.mark.parametrize("B,L", DECODES)
def test_tiny_decoder_matches_the_float64_restatement(B, L, c64, c64_everywhere, results_log):
    n = native()
    sd, z, img, ref_u8 = decoder_reference(B, L)
    net = n.NativeTinyVAEDecoder(n.TinyVAEConfig(), n.DictProvider(sd), DEV)
    prog = net.build(B, L, c64=c64)
    names = prog.prog.op_names()
    assert names[0] == "lb_nchw_to_nhwc_f16" and names[-1] == "lb_postprocess_u8" and len(names) == 2 + 35
    assert names.count("conv3x3_c64") == (33 if c64 else 0) == prog.c64_launches
    h, w = (L, L) if isinstance(L, int) else L
    assert (prog.H, prog.W, prog.L) == (h, w, L if isinstance(L, int) else None)
    assert tuple(prog.frames.shape) == (B, 8 * h, 8 * w, 3) and prog.frames.dtype == torch.uint8
    got_u8 = prog.decode(z.to(DEV)).cpu().numpy()
    _bars(results_log, f"tiny_vae_B{B}_{h}x{w}_c64{int(c64)}", prog, got_u8, img, ref_u8)
    prog.prog.instantiate()                                         # graph replay equals eager bytes
    assert np.array_equal(prog.decode(z.to(DEV)).cpu().numpy(), got_u8)


def test_tiny_decoder_loads_the_checkpoint_layout_from_safetensors(tmp_path, c64_everywhere):
    """A safetensors file with taesdxl's key names (encoder keys present and ignored) gives the bytes of the DictProvider."""
    from safetensors.torch import save_file
    n = native()
    sd, z, _, _ = decoder_reference(1, 8)
    d = tmp_path / "taesdxl"
    d.mkdir()
    save_file({**{k: v.half().contiguous() for k, v in sd.items()}, "encoder.layers.0.weight": torch.zeros(64, 3, 3, 3, dtype=F16)},
              str(d / "diffusion_pytorch_model.safetensors"))
    a = n.NativeTinyVAEDecoder(n.TinyVAEConfig(), n.from_safetensors(str(d)), DEV).build(1, 8).decode(z.to(DEV)).cpu()
    b = n.NativeTinyVAEDecoder(n.TinyVAEConfig(), n.DictProvider(sd), DEV).build(1, 8).decode(z.to(DEV)).cpu()
    assert torch.equal(a, b)
    with pytest.raises(KeyError, match="decoder.layers.18.bias"):
        n.NativeTinyVAEDecoder(n.TinyVAEConfig(), n.DictProvider({k: v for k, v in sd.items() if k != "decoder.layers.18.bias"}), DEV)


def test_emitters_rule_decides_the_bit_per_conv():
    """Under the shipped rule the bit goes on exactly the convs whose output map has at least C64_MIN_TILES tiles."""
    from latentblending_amd.native import tiny_vae
    n = native()
    net = n.NativeTinyVAEDecoder(n.TinyVAEConfig(), n.SyntheticProvider(3), DEV)
    B, L = 2, 16
    want = 0
    side = L
    for stage, blocks in enumerate((3, 3, 3, 1)):
        want += 3 * blocks * int(tiny_vae.use_c64(B, side, side))
        if stage < 3:
            side *= 2
            want += int(tiny_vae.use_c64(B, side, side))
    prog = net.build(B, L)
    assert prog.prog.op_names().count("conv3x3_c64") == want == prog.c64_launches
    assert net.build(B, L, c64=False).prog.op_names().count("conv3x3_c64") == 0


# ====================================================================== pipe and engine
def make_pipe(decoder="tiny", **kw):
    n = native()
    return n.NativeSDXLPipe(turbo=True, unet_cfg=n.UNetConfig(**dataclasses.asdict(R.tiny_unet_cfg())),
                            vae_cfg=n.VAEConfig(**dataclasses.asdict(R.tiny_vae_cfg())), seed=0, scheduler="ddim",
                            allow_synthetic=True, decoder=decoder, **kw)


def make_engine(pipe, size=(128, 128)):
    from latentblending_amd import BlendingEngine
    np.random.seed(0)
    be = BlendingEngine(pipe, verbose=False, do_compile=True)
    be.set_dimensions(size)
    be.set_num_inference_steps(4)
    be.set_branching(depth_strength=0.5, nmb_max_branches=5)
    be.set_prompt1("photo of a reef")
    be.set_prompt2("rendering of an alien planet")
    return be


def as_np(frames):
    return [np.asarray(f) for f in frames]


class StableDiffusionXLPipeline:
    """The native pipe seen as a plain diffusers pipe (DiffusersHolder dispatches on this class name): the holder then takes its
    generic latent2image path - latents / scaling_factor -> vae.decode -> image_processor.postprocess."""
    is_lb_native = False

    def __init__(self, pipe):
        self._pipe = pipe

    def __getattr__(self, name):
        return getattr(self._pipe, name)


def test_unknown_decoders_raise():
    for bad in ("medium", None, 7):
        with pytest.raises(ValueError, match="decoder"):
            make_pipe(decoder=bad)
    p = make_pipe(decoder=" TINY ")
    assert p.decoder == "tiny"
    with pytest.raises(ValueError, match="decoder"):
        p.decoder = "small"
    assert p.decoder == "tiny"


def test_transition_under_the_tiny_decoder(c64_everywhere, results_log):
    from latentblending_amd import DiffusersHolder
    n = native()
    sd = T.synthetic_state_dict(0)
    p = make_pipe("tiny", tiny_vae_provider=n.DictProvider(sd))
    assert p.vae.config.scaling_factor == 1.0 and p.vae.config.force_upcast is False
    be = make_engine(p)
    decodes = p.stats["vae_decodes"]
    frames = as_np(be.run_transition(fixed_seeds=[420, 421]))
    assert len(frames) == len(be.tree_latents) == 7 and all(f.shape == (128, 128, 3) and f.dtype == np.uint8 for f in frames)
    assert p.stats["vae_decodes"] - decodes >= len(frames)
    assert p._tiny_vae_programs and not p._vae_programs, "the full decoder must not have been built or run"
    assert all(isinstance(v, n.TinyVAEProgram) and v.c64_launches == 33 for v in p._tiny_vae_programs.values())
    # every tree frame = a direct tiny decode of that node's final latent, byte for byte; also through the generic holder path
    dh_generic = DiffusersHolder(StableDiffusionXLPipeline(p))
    for k, traj in enumerate(be.tree_latents):
        direct = np.asarray(p.native_latent2image(traj[-1]))
        assert np.array_equal(direct, frames[k]), f"tree frame {k}"
        assert np.array_equal(np.asarray(dh_generic.latent2image(traj[-1])), direct), f"generic path, frame {k}"
    # ... and the frames are the tiny decoder's: the float64 restatement of the same latents, at the decoder's bars
    z = torch.cat([t[-1].reshape(1, 4, 16, 16) for t in be.tree_latents]).cpu()
    ref_u8 = T.to_u8(T.decode(sd, z)).numpy()
    d = np.abs(np.stack(frames).astype(np.int32) - ref_u8.astype(np.int32))
    results_log["tiny_vae_transition"] = {"mean_abs_u8": float(d.mean()), "frac_within_4": float((d <= 4).mean())}
    assert d.mean() <= 2 and (d <= 4).mean() >= 0.99
    # the A/B switch drops the cached tiny programs and still meets the bars
    p.tiny_conv_c64 = False
    assert not p._tiny_vae_programs
    again = np.stack(as_np(p.native_latent2image_batch([t[-1] for t in be.tree_latents])))
    assert all(v.c64_launches == 0 for v in p._tiny_vae_programs.values()) and p._tiny_vae_programs
    d = np.abs(again.astype(np.int32) - ref_u8.astype(np.int32))
    assert d.mean() <= 2 and (d <= 4).mean() >= 0.99
    # switching to the full decoder afterwards reproduces a pipe that never saw "tiny"
    p.decoder = "full"
    assert p.vae.config.scaling_factor == p.vae_cfg.scaling_factor != 1.0
    full_after = as_np(make_engine(p).run_transition(fixed_seeds=[420, 421]))
    full_never = as_np(make_engine(make_pipe("full")).run_transition(fixed_seeds=[420, 421]))
    assert len(full_after) == len(full_never) and all(np.array_equal(a, b) for a, b in zip(full_after, full_never))
    assert not all(np.array_equal(a, b) for a, b in zip(full_after, frames))


def test_tiny_decoder_renders_non_square_sizes_and_honours_graphs(c64_everywhere):
    p = make_pipe("tiny")
    p.enable_graphs(True)
    be = make_engine(p, size=(384, 128))
    frames = as_np(be.run_transition(fixed_seeds=[420, 421]))
    assert frames and all(f.shape == (128, 384, 3) for f in frames)
    built = [(k, v.prog.graph_ready, v.H, v.W, v.L) for k, v in p._tiny_vae_programs.items()]
    nonsquare = [b for b in built if len(b[0]) == 3]                  # (the engine's constructor decodes once at its default square size)
    assert nonsquare and all(b[1] for b in built) and all(b[2:] == (16, 48, None) for b in nonsquare), built
    p.enable_graphs(False)
    eager = np.asarray(make_pipe("tiny").native_latent2image(be.tree_latents[0][-1]))
    assert np.array_equal(eager, frames[0])


def test_replay_helpers_pass_the_decoder_through_and_restore_it():
    from latentblending_amd import replay
    p = make_pipe("full")
    be = make_engine(p)
    seen = []
    segs = replay.run_multi_transition(be, ["a reef", "an alien planet"], [420, 421], None, decoder="tiny",
                                       on_segment=lambda i, frames: seen.append(p.decoder))
    assert seen == ["tiny"] and p.decoder == "full" and p._tiny_vae_programs and len(segs) == 1
    with pytest.raises(ValueError, match="decoder"):
        replay.run_multi_transition(be, ["a reef", "an alien planet"], [420, 421], None, decoder="small")
    assert p.decoder == "full"
