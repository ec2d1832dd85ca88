"""Host side of the native SDXL VAE encoder (no GPU).

1. *Pin*: the float64 / float32 restatement of ``AutoencoderKL.encode`` (tests/_vae_encoder_ref.py) against the latent-diffusion
   encoder ``transformers`` ships as ``JanusVQVAEEncoder`` - code the author of the restatement never saw - on identical weights.
2. *Mutants*: the bugs most likely to be written, each evaluated at the unit it touches, each outside the bound the GPU tests hold
   the native units to (``FACTOR`` x the storage model's own error against float64).
3. *Geometry*: ``ConvGeom.down3x3`` and where ``lb_conv_plan`` sends it.
4. *Loader*: the provider is asked for exactly the checkpoint's keys; refusals.
5. *Replay and JSON* on a fake engine; 6. *sampling* on crafted moments.
"""
import dataclasses
import json
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import _model_units as MU  # noqa: E402
import _vae_encoder_ref as ER  # noqa: E402
from oracle import sdxl_ref as R  # noqa: E402

F16, F32, F64 = torch.float16, torch.float32, torch.float64
VAE_CH = (64, 128, 128, 128)


# ====================================================================== 1. pin
def third_party_encoder(cfg: R.VAECfg, w):
    """``JanusVQVAEEncoder`` in the SDXL VAE's configuration with the oracle-style weights copied in by name.  The module also puts
    attention blocks behind the resnets of its lowest level; the SD autoencoders were trained without (``attn_resolutions = []``,
    diffusers: ``DownEncoderBlock2D`` has none), so that ModuleList is emptied - the forward then skips it."""
    import transformers.models.janus.modeling_janus as janus
    from transformers.models.janus.configuration_janus import JanusVQVAEConfig
    base = cfg.block_channels[0]
    assert all(c % base == 0 for c in cfg.block_channels)
    jc = JanusVQVAEConfig(base_channels=base, channel_multiplier=[c // base for c in cfg.block_channels],
                          num_res_blocks=cfg.layers_per_block, latent_channels=cfg.latent_channels, in_channels=cfg.out_channels,
                          double_latent=True, dropout=0.0)
    enc = janus.JanusVQVAEEncoder(jc).float().eval()
    enc.down[-1].attn = torch.nn.ModuleList()

    def put(param, value):
        assert tuple(param.shape) == tuple(value.shape), (tuple(param.shape), tuple(value.shape))
        param.data.copy_(value.float())

    def conv(mod, key):
        put(mod.weight, w[key + ".weight"])
        put(mod.bias, w[key + ".bias"])

    def lin_as_conv(mod, key):
        put(mod.weight, w[key + ".weight"][:, :, None, None])
        put(mod.bias, w[key + ".bias"])

    def resnet(mod, key):
        for name in ("norm1", "conv1", "norm2", "conv2"):
            conv(getattr(mod, name), f"{key}.{name}")
        if key + ".conv_shortcut.weight" in w:
            conv(mod.nin_shortcut, key + ".conv_shortcut")
        else:
            assert not hasattr(mod, "nin_shortcut")

    conv(enc.conv_in, "encoder.conv_in")
    for bi, down in enumerate(enc.down):
        assert len(down.block) == cfg.layers_per_block
        for li, blk in enumerate(down.block):
            resnet(blk, f"encoder.down_blocks.{bi}.resnets.{li}")
        if bi < len(enc.down) - 1:
            conv(down.downsample.conv, f"encoder.down_blocks.{bi}.downsamplers.0.conv")
        else:
            assert not hasattr(down, "downsample")
    resnet(enc.mid.block_1, "encoder.mid_block.resnets.0")
    conv(enc.mid.attn_1.norm, ER.A_ENC + ".group_norm")
    for mine, theirs in (("to_q", "q"), ("to_k", "k"), ("to_v", "v"), ("to_out.0", "proj_out")):
        lin_as_conv(getattr(enc.mid.attn_1, theirs), f"{ER.A_ENC}.{mine}")
    resnet(enc.mid.block_2, "encoder.mid_block.resnets.1")
    conv(enc.norm_out, "encoder.conv_norm_out")
    conv(enc.conv_out, "encoder.conv_out")
    # the module's parameter count is the enumeration's (quant_conv is no part of the LDM encoder class)
    n_theirs = sum(p.numel() for p in enc.parameters())
    n_mine = sum(int(torch.tensor(shape).prod()) for name, shape, _, _ in ER.encoder_spec(cfg).items if not name.startswith("quant_conv"))
    assert n_theirs == n_mine == sum(v.numel() for k, v in w.items() if not k.startswith("quant_conv")), (n_theirs, n_mine)
    return enc


@pytest.mark.parametrize("which,H,W", [("tiny", 48, 80), ("sdxl", 64, 64)])
def test_restatement_equals_the_third_party_ldm_encoder(which, H, W):
    """Same weights, same picture: bar = the decoder pin's own (tests/test_oracle_pins_cpu.py), rel-L2 < 2e-5 and max < 1e-3 of
    the peak; measured 7.8e-7."""
    cfg = R.tiny_vae_cfg() if which == "tiny" else R.VAECfg()
    w = {k: v.float() for k, v in R.make_weights(ER.encoder_spec(cfg), seed=1).items()}
    enc = third_party_encoder(cfg, w)
    x = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(5)) * 2 - 1
    with torch.no_grad():
        mine = ER.encode_ref(cfg, w, x)
        theirs = torch.nn.functional.conv2d(enc(x), w["quant_conv.weight"], w["quant_conv.bias"])
    assert mine.shape == theirs.shape == (2, 2 * cfg.latent_channels, H // 8, W // 8)
    err = float((mine - theirs).norm() / theirs.norm())
    print(f"[vae-encoder] pin {which}: rel-L2 {err:.2e}")
    assert err < 2e-5, err
    assert float((mine - theirs).abs().max()) < 1e-3 * float(theirs.abs().max())
    if which == "tiny":     # the pin sees the bug most likely to be written
        with torch.no_grad():
            sym = ER.encode_ref(cfg, w, x, pad="sym")
        assert float((sym - theirs).norm() / theirs.norm()) > 0.1


# ====================================================================== 2. mutants
def outside(value, model, ref64):
    """``MU.compare``'s verdict on ``value``: True when it is OUTSIDE FACTOR x the storage model's own error (either norm)."""
    m_l2, m_max = MU.errors(model, ref64)
    v_l2, v_max = MU.errors(value, ref64)
    assert m_l2 > 0 and m_max > 0
    print(f"[vae-encoder] mutant: l2 {v_l2:.3e} (model {m_l2:.3e}) max {v_max:.3e} (model {m_max:.3e})")
    return not (v_l2 <= MU.FACTOR * m_l2 and v_max <= MU.FACTOR * m_max)


@pytest.fixture(scope="module")
def units():
    """The float64 free run of a 32 x 48 picture at the GPU tests' widths: every unit's input, computed once."""
    cfg = R.VAECfg(block_channels=VAE_CH)
    w = R.make_weights(ER.encoder_spec(cfg), 1)
    ref, model = MU.evs(w)
    x = ER.picture(torch.randint(0, 256, (2, 32, 48, 3), generator=torch.Generator().manual_seed(7), dtype=torch.uint8))
    return SimpleNamespace(cfg=cfg, w=w, ref=ref, model=model, x=x, run=ER.free_run(ref, cfg, x))


def test_chained_units_are_the_restatement(units):
    u = units
    taps = {}
    want = ER.encode_ref(u.cfg, u.w, u.x, taps=taps, dtype=F64)
    assert torch.allclose(u.run["moments"], want, rtol=0, atol=1e-10)
    for tap, unit in ER.encoder_tap_names(u.cfg).items():
        assert torch.allclose(u.run[unit], taps[tap], rtol=0, atol=1e-9), tap
    assert torch.allclose(u.run["latents"], want[:, :4] * u.cfg.scaling_factor, rtol=0, atol=1e-12)
    for scaled in (True, False):        # the storage model is the same function up to its roundings
        m = ER.free_run(u.model, u.cfg, u.x, scaled=scaled)
        l2, _ = MU.errors(m["latents"], u.run["latents"])
        assert 0 < l2 < 1e-2, (scaled, l2)
        assert not outside(m["latents"], m["latents"], u.run["latents"])


@pytest.mark.parametrize("pad", ["sym", "tl"])
@pytest.mark.parametrize("scaled", [True, False])
def test_mutant_downsampler_padding(units, pad, scaled):
    u = units
    for bi in range(3):
        p = f"encoder.down_blocks.{bi}.downsamplers.0.conv"
        x = u.run[f"encoder.down_blocks.{bi}.resnets.1"]
        ref64 = ER.downsample_unit(u.ref, x, p, scaled)
        assert torch.equal(ref64, torch.nn.functional.conv2d(torch.nn.functional.pad(x, (0, 1, 0, 1)), u.ref.w[p + ".weight"],
                                                             u.ref.w[p + ".bias"], stride=2))
        model = ER.downsample_unit(u.model, u.model.t(x), p, scaled)
        assert not outside(model, model, ref64)
        assert outside(ER.downsample_unit(u.model, u.model.t(x), p, scaled, pad=pad), model, ref64), (bi, pad)


def test_mutants_of_the_moments(units):
    u = units
    x = u.run["encoder.mid_block.resnets.1"]
    ref64 = ER.moments_unit(u.ref, u.cfg, x)
    model = ER.moments_unit(u.model, u.cfg, u.model.t(x))
    assert not outside(model, model, ref64)
    # mean and logvar halves swapped
    assert outside(torch.cat(list(reversed(model.chunk(2, dim=1))), dim=1), model, ref64)
    # quant_conv left out
    n = MU.gn(u.model, u.model.t(x), "encoder.conv_norm_out", u.cfg.norm_groups, 1e-6, True)
    assert outside(R._conv(n, u.model.w, "encoder.conv_out"), model, ref64)


def test_mutant_fold_in_fp16(units):
    """W' = Wq Wout summed in fp16 arithmetic rounds every partial sum at the partial sum's magnitude; the loader's float64 fold rounds
    the result once, at its own.  The two differ by a factor wherever the sum cancels, and only there: on the seeded stand-in weights
    (eight terms of like size) the fp16 fold measures 1.65x the storage model's error - inside FACTOR, not a detectable bug - so this
    mutant is run on a quant_conv / conv_out pair whose first two terms cancel to 2^-6 of their size, each weighted about 33: the
    products then carry a rounding error of 2^-12 * 33 |Wout| into a result of about |Wout|, some thirty times the single rounding
    (measured: 32x the storage model's rel-L2)."""
    u = units
    w = dict(u.w)
    wo, bo, wq = w["encoder.conv_out.weight"].clone(), w["encoder.conv_out.bias"].clone(), w["quant_conv.weight"].clone()
    wo[1] = (-wo[0] + 2.0 ** -6 * wo[1]).half().float()
    bo[1] = (-bo[0] + 2.0 ** -6 * bo[1]).half().float()
    wq[:, 0] = wq[:, 1] = torch.linspace(29.0, 37.0, 8).half().float()[:, None, None]      # (no powers of two: their products are exact)
    w.update({"encoder.conv_out.weight": wo, "encoder.conv_out.bias": bo, "quant_conv.weight": wq})
    ref, model_ev = MU.evs(w)
    x = u.run["encoder.mid_block.resnets.1"]
    ref64 = ER.moments_unit(ref, u.cfg, x)
    model = ER.moments_unit(model_ev, u.cfg, model_ev.t(x))
    assert not outside(model, model, ref64)
    assert outside(ER.moments_unit(model_ev, u.cfg, model_ev.t(x), fold="f16"), model, ref64)
    # ... and on any weights the loader test holds the packed tensor to the float64 fold bit for bit, which no fp16 fold meets
    a, b = ER.folded_moments_weights(u.w)[0], ER.folded_moments_weights(u.w, fold="f16")[0]
    assert not torch.equal(a, b)


def test_mutant_scaling_factor_left_out(units):
    u = units
    m = u.run["moments"].to(F32)
    ref64 = ER.latents_unit(u.ref, u.cfg, m)
    model = ER.latents_unit(u.model, u.cfg, m)
    assert not outside(model, model, ref64)
    assert outside(ER.latents_unit(u.model, u.cfg, m, scale=False), model, ref64)


def test_mutant_groupnorm_eps(units):
    """eps 1e-5 instead of 1e-6 moves a normalised value by (1e-5 - 1e-6) / (2 var): it shows where a group's variance is small.  A
    picture of amplitude 2^-7 around mid-grey: conv_in's groups (two channels each) then vary by about the spread of two biases, 1e-3 and
    less - the first resnet is the unit to look at (the UNet tests use a quiet latent for the same reason)."""
    u = units
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(2, 3, 32, 48, generator=g) * 2.0 ** -7).to(F16)
    p = "encoder.down_blocks.0.resnets.0"
    h = ER.encoder_unit(u.ref, u.cfg, "conv_in", "conv_in", [x], True)
    ref64 = MU.vae_resnet(u.ref, u.cfg, p, h, True)
    model = MU.vae_resnet(u.model, u.cfg, p, u.model.t(h), True)
    assert not outside(model, model, ref64)
    assert outside(R.resnet_block(h, None, u.ref.w, p, u.cfg.norm_groups, 1e-5), model, ref64)


# ====================================================================== 3. geometry
def test_down3x3_geometry_and_its_route():
    from latentblending_amd.hip import lib
    g = lib.ConvGeom.down3x3(12, 20, 128)
    assert (g.Hin, g.Win, g.Cin, g.KH, g.KW, g.stride, g.pad, g.ups, g.ldx, g.parity, g.Hout, g.Wout) == (12, 20, 128, 3, 3, 2, 0, 0, 128, None, 6, 10)
    assert g.M(3) == 180 and g.K == 9 * 128 and g.scatter == 0 and isinstance(g, lib.ConvGeom) and len(g) == 12
    assert lib.ConvGeom.down3x3(12, 20, 128, ldx=136).ldx == 136
    assert lib.ConvGeom(12, 20, 128, 3, 3, 2, 0).Hout == 5, "the general constructor cannot express it: that is why down3x3 exists"
    for H, W in ((11, 20), (12, 21), (0, 4), (-2, 4)):
        with pytest.raises(ValueError, match="even"):
            lib.ConvGeom.down3x3(H, W, 128)
    p = lib.gemm_params(M=g.M(3), N=128, K=g.K, ldw=g.K, ldc=128, conv=g, zero_page=64)
    assert (p.conv, p.Hin, p.Win, p.Cin, p.KH, p.KW, p.stride, p.pad, p.ups, p.ldx, p.Hout, p.Wout, p.scatter) == \
        (1, 12, 20, 128, 3, 3, 2, 0, 0, 128, 6, 10, 0)
    # every other conv route refuses stride 2 / pad 0: the implicit GEMM, at the SDXL widths and with every opt-in bit the emitter sets
    for c in (128, 256, 512):
        for H, W in ((64, 64), (512, 512), (96, 160)):
            for halo in (1, 2):
                lib.api.lb_gemm_set_halo(halo)
                try:
                    for flags in (0, lib.GEMM_HALO_KSPLIT, lib.GEMM_HALO_RAGGED, lib.GEMM_OUT_F32):
                        g = lib.ConvGeom.down3x3(H, W, c)
                        plan = lib.conv_plan(lib.gemm_params(M=g.M(2), N=c, K=g.K, ldw=g.K, ldc=c, conv=g, flags=flags, zero_page=64))
                        assert plan.route == lib.ROUTE_GEMM and plan.halo_kind == 0 and plan.ragged_kind == 0 and plan.stat_rows == 0
                        assert plan.gn_a_fuse == 0 and plan.ksplit_split == 0 and plan.tile > 0 and plan.blocks > 0
                finally:
                    lib.api.lb_gemm_set_halo(1)
    # a narrow output (N <= 16) is no way round it either
    g = lib.ConvGeom.down3x3(64, 64, 128)
    assert lib.conv_plan(lib.gemm_params(M=g.M(2), N=8, K=g.K, ldw=g.K, ldc=8, conv=g, zero_page=64)).route == lib.ROUTE_GEMM


# ====================================================================== 4. loader
class Spy:
    def __init__(self, inner):
        self.inner, self.asked = inner, []

    def weight(self, name, shape, fan_in=0, gain=1.0):
        self.asked.append(name)
        return self.inner.weight(name, shape, fan_in, gain)

    def bias(self, name, n):
        self.asked.append(name)
        return self.inner.bias(name, n)

    def norm_weight(self, name, n):
        self.asked.append(name)
        return self.inner.norm_weight(name, n)


@pytest.mark.parametrize("ch", [VAE_CH, (32, 64, 64, 512)])
def test_loader_asks_for_exactly_the_checkpoint_keys(ch):
    import latentblending_amd.native as n
    from latentblending_amd.native import vae as V
    cfg = n.VAEConfig(block_channels=ch)
    spy = Spy(n.SyntheticProvider(1))
    net = n.NativeVAEEncoder(cfg, spy, "cpu")
    keys = V.encoder_state_dict_keys(cfg)
    assert spy.asked == keys and len(set(keys)) == len(keys)
    assert keys == [name for name, _, _, _ in ER.encoder_spec(R.VAECfg(block_channels=ch)).items]
    # the synthetic stand-in and the oracle-style weights are the same tensors: the GPU tests rely on it
    w = R.make_weights(ER.encoder_spec(R.VAECfg(block_channels=ch)), 1)
    state = n.NativeVAEEncoder(cfg, n.DictProvider(w), "cpu").w
    assert list(state) == list(net.w) and all(torch.equal(state[k], net.w[k]) for k in state)
    # layouts: conv_in's Cin 3 padded to 8, the folded moments conv, biases in stream units, the fused qkv at 512
    top = ch[-1]
    assert tuple(net.w["encoder.conv_in.weight"].shape) == (ch[0], 9 * 8) and net.w["encoder.conv_in.weight"].dtype == F16
    assert tuple(net.w["encoder.moments.weight"].shape) == (8, 9 * top) and net.w["encoder.moments.bias"].dtype == F32
    assert "quant_conv.weight" not in net.w and "encoder.conv_out.weight" not in net.w
    wf, bf = ER.folded_moments_weights({k: v.double() for k, v in w.items()})
    assert torch.equal(net.w["encoder.moments.weight"].double().view(8, 3, 3, top).permute(0, 3, 1, 2), wf)
    assert torch.equal(net.w["encoder.moments.bias"].double(), bf)
    assert all(torch.equal(net.w[k + "_s"], net.w[k] / 16) for k in net.w if k.endswith(".bias"))
    assert ((ER.A_ENC + ".qkv.weight") in net.w) == (top == 512)
    assert tuple(net.w["encoder.down_blocks.1.downsamplers.0.conv.weight"].shape) == (ch[1], 9 * ch[1])


def test_default_key_list_is_the_sdxl_checkpoint():
    from latentblending_amd.native import vae as V
    keys = V.encoder_state_dict_keys()
    assert len(keys) == 108 and keys[:2] == ["encoder.conv_in.weight", "encoder.conv_in.bias"] and keys[-2:] == ["quant_conv.weight", "quant_conv.bias"]
    assert "encoder.down_blocks.1.resnets.0.conv_shortcut.weight" in keys and "encoder.down_blocks.2.resnets.0.conv_shortcut.weight" in keys
    assert sum(k.endswith("conv_shortcut.weight") for k in keys) == 2 and not any("down_blocks.3.downsamplers" in k for k in keys)
    assert not any(".attentions." in k and "down_blocks" in k for k in keys)
    spec = ER.encoder_spec(R.VAECfg())
    assert keys == [name for name, _, _, _ in spec.items]
    assert R.count_params(spec) - 8 * 8 - 8 == 34_163_592, "the encoder.* parameters of the SDXL VAE"


def test_a_missing_key_is_named():
    import latentblending_amd.native as n
    w = R.make_weights(ER.encoder_spec(R.VAECfg(block_channels=VAE_CH)), 1)
    del w["quant_conv.weight"]
    with pytest.raises(KeyError, match="quant_conv.weight"):
        n.NativeVAEEncoder(n.VAEConfig(block_channels=VAE_CH), n.DictProvider(w), "cpu")


def test_pipe_refusals_need_no_device():
    import latentblending_amd.native as n
    with pytest.raises(ValueError, match="encoder must be 'tiny' or 'full'.*bogus"):
        n.NativeSDXLPipe(encoder="bogus")
    with pytest.raises(ValueError, match="encoder must be"):
        n.NativeSDXLPipe(encoder=None)
    decoder = SimpleNamespace(cfg=n.VAEConfig())
    with pytest.raises(ValueError, match="vae_native=.*vae_provider="):
        n.NativeSDXLPipe(encoder="full", vae_native=decoder)
    # the lazy path refuses the same way (the default pipe accepts a ready-made decoder as ever, until the full encoder is asked for)
    shell = n.NativeSDXLPipe.__new__(n.NativeSDXLPipe)
    shell._encoder, shell._vae_provider, shell._vae_native_given, shell.vae_encoder_native, shell._vae_seed = "tiny", None, True, None, 1
    with pytest.raises(ValueError, match="never paired"):
        shell.encoder = "full"
    assert shell.encoder == "tiny"
    with pytest.raises(ValueError, match="never paired"):
        shell._vae_encoder_net()
    shell._vae_native_given = False
    shell.encoder = " Full "
    assert shell.encoder == "full" and isinstance(shell._full_encoder_source(), n.SyntheticProvider)
    shell.vae_encoder_native = object()
    shell._vae_native_given = True
    assert shell._full_encoder_source() is None and shell._vae_encoder_net() is shell.vae_encoder_native


@pytest.mark.parametrize("B,L,kw", [(2, 16, {}), (3, (12, 20), {}), (2, (8, 16), {"stream_fp16_scaled": False})])
def test_program_journal_and_marks_recorded_on_the_cpu(monkeypatch, B, L, kw):
    """The encode program recorded without a device (nothing is launched): marks, taps and the arena's ledger, under the default
    routes and with every eligible conv on the halo kernel."""
    import latentblending_amd.native as n
    import latentblending_amd.native.runtime as rt
    import latentblending_amd.native.vae as V
    from latentblending_amd.hip import lib
    from test_model_units_cpu import _ledger
    for mod in (rt, V):
        monkeypatch.setattr(mod, "_stream", lambda: None)
    cfg = R.VAECfg(block_channels=VAE_CH)
    net = n.NativeVAEEncoder(n.VAEConfig(**dataclasses.asdict(cfg), **kw), n.SyntheticProvider(1), "cpu")
    H, W = (L, L) if isinstance(L, int) else L
    for halo in (1, 2):
        lib.api.lb_gemm_set_halo(halo)
        try:
            plain, prog = net.build(B, L), net.build(B, L, journal=True)
        finally:
            lib.api.lb_gemm_set_halo(1)
        assert plain.arena.journal is None and prog.prog.op_names() == plain.prog.op_names()
        assert [len(t) for t in plain.arena.all] == [len(t) for t in prog.arena.all]
        progs = {prog.prog.name: prog.prog}
        _ledger(prog, progs)
        assert prog.persistent == []
        MU.check_marks(prog.marks, progs, ("x_in",))
        assert [(m.name, m.kind, m.inputs) for m in prog.marks] == ER.encoder_units(cfg)
        assert prog.tap_names == ER.encoder_tap_names(cfg)
        assert [m.op_end for m in plain.marks] == [m.op_end for m in prog.marks]
        assert prog.marks[-1].op_end == prog.prog.num_ops - 2 and prog.marks[-1].out is prog.moments_f32   # (then: cast, layout)
        assert tuple(prog.x_in.shape) == (B, 8 * H, 8 * W, 8) and tuple(prog.latents.shape) == (B, 4, H, W)
        assert tuple(prog.marks[0].out.shape) == (B, 8 * H, 8 * W, 64) and tuple(prog.marks[-2].out.shape) == (B, H, W, 128)
        names = prog.prog.op_names()
        downs = [i for i, m in enumerate(prog.marks) if m.kind == "downsample"]
        assert len(downs) == 3 and all(names[prog.marks[i].op_end - 1] == "lb_gemm_f16" for i in downs)


# ====================================================================== 5. replay and JSON
class FakePipe:
    def __init__(self):
        self._encoder, self.sets = "tiny", []

    @property
    def encoder(self):
        return self._encoder

    @encoder.setter
    def encoder(self, name):
        if name not in ("tiny", "full"):
            raise ValueError(name)
        self.sets.append(name)
        self._encoder = name


class FakeEngine:
    """The engine calls the replay drivers make, recorded; ``run_transition`` notes which encoder the pipe is on."""

    def __init__(self, pipe):
        self.dh = SimpleNamespace(pipe=pipe, width_img=128, height_img=96, num_inference_steps=4)
        self.seen, self.anchors = [], []

    def set_prompt1(self, p): pass
    def set_prompt2(self, p): pass
    def set_negative_prompt(self, p): pass
    def swap_forward(self): pass
    def clear_anchor_images(self): pass
    def set_dimensions(self, size): self.dh.width_img, self.dh.height_img = size
    def set_num_inference_steps(self, n): self.dh.num_inference_steps = n
    def set_anchor_image1(self, im, s): self.anchors.append((1, self.dh.pipe.encoder))
    def set_anchor_image2(self, im, s): self.anchors.append((2, self.dh.pipe.encoder))

    def run_transition(self, **kw):
        self.seen.append(self.dh.pipe.encoder)
        return ["frame"]


def test_replay_passes_the_encoder_through_and_restores_it():
    from latentblending_amd import replay
    pipe = FakePipe()
    be = FakeEngine(pipe)
    replay.run_multi_transition(be, ["a", "b", "c"], [1, 2, 3], None, list_images=[None, "picture", None], image_encoder="full")
    assert be.seen == ["full", "full"] and be.anchors == [(2, "full")] and pipe.encoder == "tiny" and pipe.sets == ["full", "tiny"]
    pipe.sets.clear()
    replay.run_multi_transition(be, ["a", "b"], [1, 2], None)
    assert pipe.sets == [] and be.seen[-1] == "tiny", "None leaves the pipe alone"
    pipe.encoder = "full"
    replay.run_multi_transition(be, ["a", "b"], [1, 2], None, image_encoder="tiny")
    assert be.seen[-1] == "tiny" and pipe.encoder == "full"
    pipe.encoder = "tiny"

    class Boom(Exception):
        pass

    def boom(**kw):
        raise Boom()
    be.run_transition = boom
    with pytest.raises(Boom):
        replay.run_multi_transition(be, ["a", "b"], [1, 2], None, image_encoder="full")
    assert pipe.encoder == "tiny", "restored after a failure too"
    with pytest.raises(ValueError):
        replay.run_multi_transition(be, ["a", "b"], [1, 2], None, image_encoder="bogus")
    other = FakeEngine(SimpleNamespace())
    with pytest.raises(ValueError, match="native pipe"):
        replay.run_multi_transition(other, ["a", "b"], [1, 2], None, image_encoder="full")


def test_movie_json_header_round_trip_and_default_writes_no_key(tmp_path):
    from latentblending_amd import replay
    pipe = FakePipe()
    be = FakeEngine(pipe)
    items = [{"iteration": i, "seed": i, "prompt": t, "negative_prompt": ""} for i, t in enumerate(["a", "b"])]
    fp = str(tmp_path / "m.json")
    # the default: the file written before this key existed, byte for byte
    replay.save_movie_json(fp, be, items)
    with open(fp) as fh:
        text = fh.read()
    header = {"settings": "sdxl", "width": 128, "height": 96, "num_inference_steps": 4}
    assert text == json.dumps([header] + items, indent=4) and "image_encoder" not in text
    replay.save_movie_json(fp, be, items, image_encoder="tiny")
    with open(fp) as fh:
        assert fh.read() == text
    replay.run_movie_json(be, fp)
    assert pipe.sets == [] and be.seen == ["tiny"]
    # the pipe's own setting is what a plain save records; an argument overrides it
    pipe.encoder = "full"
    replay.save_movie_json(fp, be, items)
    assert replay.load_movie_json(fp)[0]["image_encoder"] == "full"
    pipe.encoder = "tiny"
    replay.save_movie_json(fp, be, items, image_encoder="Full")
    head, back = replay.load_movie_json(fp)
    assert head == {**header, "image_encoder": "full"} and back == items
    with pytest.raises(ValueError, match="image_encoder"):
        replay.save_movie_json(fp, be, items, image_encoder="bogus")
    # the header key selects the encoder for the movie and the pipe is restored; the argument beats the header
    pipe.sets.clear()
    replay.run_movie_json(be, fp)
    assert be.seen[-1] == "full" and pipe.encoder == "tiny" and pipe.sets == ["full", "tiny"]
    replay.run_movie_json(be, fp, image_encoder="tiny")
    assert be.seen[-1] == "tiny" and pipe.encoder == "tiny"
    # a pipe without the switch writes the default file
    replay.save_movie_json(fp, FakeEngine(SimpleNamespace()), items)
    with open(fp) as fh:
        assert fh.read() == text


# ====================================================================== 6. sampling
def test_sampling_on_crafted_moments():
    from latentblending_amd.native.vae import sample_moments
    g = torch.Generator().manual_seed(3)
    mean = torch.randn(2, 3, 5, 4, generator=g)
    logvar = torch.randn(2, 3, 5, 4, generator=g) * 3
    logvar[0, 0, 0] = torch.tensor([-100.0, 100.0, -30.0, 20.0])
    logvar[1, 2, 4] = torch.tensor([-31.0, 21.0, 0.0, float(2 ** -20)])
    moments = torch.cat([mean, logvar], dim=-1)             # channels last, as the program leaves them
    eps = torch.randn(2, 3, 5, 4, generator=g)
    got = sample_moments(moments, eps=eps)
    want = ER.sample_ref(moments.double().permute(0, 3, 1, 2), eps.double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    assert got.dtype == F32 and torch.isfinite(got).all()
    # fp32 arithmetic: exp of an fp32 argument up to 10 carries a relative error of a few ulp, the product and the sum one each
    assert float(((got.double() - want).abs() / (want.abs() + eps.double().abs() * torch.exp(0.5 * logvar.double().clamp(-30, 20)))).max()) < 1e-6
    # the clamps: logvar -100 is std e^-15, +100 is std e^10 - not e^-50 / e^50
    std = ((got - mean) / eps).double()
    assert abs(float(std[0, 0, 0, 0]) / torch.exp(torch.tensor(-15.0, dtype=F64)).item() - 1) < 1e-2 or abs(float(got[0, 0, 0, 0] - mean[0, 0, 0, 0])) < 1e-6
    assert abs(float(std[0, 0, 0, 1]) / torch.exp(torch.tensor(10.0, dtype=F64)).item() - 1) < 1e-5
    assert abs(float(std[1, 2, 4, 1]) / torch.exp(torch.tensor(10.0, dtype=F64)).item() - 1) < 1e-5
    # the generator path draws on the moments' device, reproducibly, and eps = 0 gives the mean
    a = sample_moments(moments, torch.Generator().manual_seed(9))
    b = sample_moments(moments, torch.Generator().manual_seed(9))
    assert torch.equal(a, b) and not torch.equal(a, got)
    assert torch.equal(sample_moments(moments, eps=torch.zeros_like(eps)), mean)
