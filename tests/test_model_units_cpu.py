"""The unit marks and the arena journal of the UNet / VAE programs, recorded on the CPU (nothing is launched), and the unit
references of tests/_model_units.py against the oracle they are built from."""
import dataclasses

import pytest
import torch

import _model_units as MU
from oracle import sdxl_ref as R

VAE_CH = (64, 128, 128, 128)


@pytest.fixture
def cpu_native(monkeypatch):
    """The native package with every launch stream replaced by None: ``build`` records on the CPU."""
    import latentblending_amd.native as n
    import latentblending_amd.native.runtime as rt
    import latentblending_amd.native.unet as U
    import latentblending_amd.native.vae as V
    for mod in (rt, U, V):
        monkeypatch.setattr(mod, "_stream", lambda: None)
    return n


def _unet(n, cfg=None, **kw):
    cfg = cfg or R.tiny_unet_cfg()
    return cfg, n.NativeUNet(n.UNetConfig(**dataclasses.asdict(cfg)), n.SyntheticProvider(0), "cpu", **kw)


def _vae(n, **kw):
    cfg = R.VAECfg(block_channels=VAE_CH)
    return cfg, n.NativeVAEDecoder(n.VAEConfig(**dataclasses.asdict(cfg), **kw), n.SyntheticProvider(1), "cpu")


def _ledger(prog, progs):
    """The journal invariants of one recorded program object."""
    ar = prog.arena
    assert ar.journal, "journal=True must record"
    live, _ = MU.journal_state(ar.journal, len(ar.all))             # double release, release before alloc, alloc while live
    assert all(name in progs and 0 <= op <= progs[name].num_ops for _, _, name, op in ar.journal), "an entry outside a recording"
    ops = {}
    for _, _, name, op in ar.journal:                               # the clock never runs backwards
        assert op >= ops.get(name, 0)
        ops[name] = op
    want = {ar._ids[id(t._lb_raw)] for t in prog.persistent}
    assert live == want, f"live at the end of emission: {sorted(live)}, persistent: {sorted(want)}"
    assert len(ar.free) and sum(len(v) for v in ar.free.values()) == len(ar.all) - len(want)


@pytest.mark.parametrize("B,L,fuse", [(2, 16, "auto"), (3, (16, 24), False), (2, (8, 16), True)])
def test_unet_journal_and_marks(cpu_native, B, L, fuse):
    cfg, net = _unet(cpu_native, fuse_layernorm=fuse)
    plain, prog = net.build(B, L), net.build(B, L, journal=True)
    assert plain.arena.journal is None
    assert prog.prog_step.op_names() == plain.prog_step.op_names() and prog.prog_cond.op_names() == plain.prog_cond.op_names()
    assert [len(t) for t in plain.arena.all] == [len(t) for t in prog.arena.all]
    progs = {p.name: p for p in (prog.prog_cond, prog.prog_step)}
    assert len(progs) == 2
    _ledger(prog, progs)
    assert len(prog.persistent) == 1 and prog.persistent[0] is prog.temb_all
    for pr in (plain, prog):
        MU.check_marks(pr.marks, progs, ("x_in", "tvals", "ctx", "text_embeds", "time_ids"))
        assert [(m.name, m.kind, m.inputs) for m in pr.marks] == MU.unet_units(cfg)
        assert pr.tap_names == MU.unet_tap_names(cfg)
        assert [m.op_end for m in pr.marks if m.program == "unet-cond"][-1] == pr.prog_cond.num_ops
        assert pr.marks[-1].op_end == pr.prog_step.num_ops and pr.marks[-1].out is pr.eps
    assert [m.op_end for m in plain.marks] == [m.op_end for m in prog.marks]
    H, W = (L, L) if isinstance(L, int) else L
    by = {m.name: m for m in prog.marks}
    assert tuple(by["conv_in"].out.shape) == (B, H, W, 64) and tuple(by["mid_block.resnets.1"].out.shape) == (B, H // 4, W // 4, 256)
    assert tuple(by["temb_all"].out.shape) == (B, net.n_temb) and tuple(by["ctx_kv"].out.shape) == (B * 80, 2 * net.n_ctx)
    # the helper's column layout of the fused projections, derived from the oracle's enumeration, is the net's
    temb, nt, ctx, nc = MU.unet_layout(cfg)
    assert (temb, nt, ctx, nc) == (net.temb_slices, net.n_temb, net.ctx_slices, net.n_ctx)


def test_unet_marks_of_a_guidance_embedded_config(cpu_native):
    cfg, net = _unet(cpu_native, dataclasses.replace(R.tiny_unet_cfg(), time_cond_proj_dim=32))
    prog = net.build(2, 16, journal=True)
    progs = {p.name: p for p in (prog.prog_cond, prog.prog_step)}
    _ledger(prog, progs)
    MU.check_marks(prog.marks, progs, ("x_in", "tvals", "ctx", "text_embeds", "time_ids", "timestep_cond"))
    assert [(m.name, m.kind, m.inputs) for m in prog.marks] == MU.unet_units(cfg, guided=True)


@pytest.mark.parametrize("B,L,kw", [(2, 16, {}), (3, (16, 24), {}), (2, (8, 16), {"stream_fp16_scaled": False}),
                                    (2, 16, {"fused_mid_attention": False})])
def test_vae_journal_and_marks(cpu_native, B, L, kw):
    from latentblending_amd.hip import lib
    cfg, net = _vae(cpu_native, **kw)
    for halo in (1, 2):                     # the default routes, and every eligible conv on the halo kernel (statistics buffers ride)
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
        MU.check_marks(prog.marks, progs, ("z_in",))
        assert [(m.name, m.kind, m.inputs) for m in prog.marks] == MU.vae_units(cfg)
        assert prog.tap_names == MU.vae_tap_names(cfg)
        assert [m.op_end for m in plain.marks] == [m.op_end for m in prog.marks]
        assert prog.marks[-1].op_end == prog.prog.num_ops - 1 and prog.marks[-1].out is prog.image_f32     # (then: the uint8 frames)
        H, W = (L, L) if isinstance(L, int) else L
        assert tuple(prog.marks[0].out.shape) == (B, H, W, 128) and tuple(prog.marks[-2].out.shape) == (B, 8 * H, 8 * W, 64)


def test_the_ledger_notices_what_it_is_there_for():
    ok = [("alloc", 0, "p", 0), ("alloc", 1, "p", 0), ("release", 0, "p", 2), ("alloc", 0, "p", 2), ("release", 1, "p", 3)]
    assert MU.journal_state(ok, 2) == ({0}, set())
    assert MU.journal_state(ok, 2, upto=("p", 0)) == ({0, 1}, {0, 1})
    assert MU.journal_state(ok, 2, upto=("p", 1)) == ({0, 1}, set())
    assert MU.journal_state(ok, 2, upto=("p", 2)) == ({0, 1}, {0})
    with pytest.raises(AssertionError, match="released twice"):
        MU.journal_state(ok + [("release", 1, "p", 4)], 2)
    with pytest.raises(AssertionError, match="without having been allocated"):
        MU.journal_state([("release", 1, "p", 0)], 2)
    with pytest.raises(AssertionError, match="while live"):
        MU.journal_state(ok + [("alloc", 0, "p", 5)], 2)


# ---------------------------------------------------------------- the unit references, chained, are the oracle
def _free_run(ev, cfg, units, unit_fn, inputs):
    """Every unit fed with the OUTPUTS OF THE SAME EVALUATION (no teacher): what the whole model computes."""
    out = dict(inputs)
    for name, kind, ins in units:
        out[name] = unit_fn(ev, cfg, name, kind, [out[i] for i in ins])
    return out


def test_chained_unet_units_are_the_oracle_forward():
    cfg = R.tiny_unet_cfg()
    w = R.make_weights(R.unet_spec(cfg), 0)
    ref, _ = MU.evs(w)
    g = torch.Generator().manual_seed(3)
    B, H, W = 2, 8, 16
    x = torch.randn(B, 4, H, W, generator=g).half()
    ctx = torch.randn(B, 77, cfg.cross_dim, generator=g).half()
    te = torch.randn(B, cfg.pooled_dim, generator=g).half()
    ids = torch.tensor([[128.0, 96.0, 0.0, 0.0, 128.0, 96.0]] * B)
    taps = {}
    want = R.unet_forward(cfg, ref.w, x, torch.tensor(499.0), ctx, te, ids, taps=taps, dtype=torch.float64)
    assert want.dtype == torch.float64 and taps["mid"].dtype == torch.float64
    got = _free_run(ref, cfg, MU.unet_units(cfg), lambda *a: MU.unet_unit(*a, fused_ln=False),
                    dict(x_in=x, tvals=torch.full((B,), 499.0), ctx=ctx, text_embeds=te, time_ids=ids))
    assert torch.allclose(got["eps"], want, rtol=0, atol=1e-11)
    for tap, unit in MU.unet_tap_names(cfg).items():
        assert torch.allclose(got[unit], taps[tap], rtol=0, atol=1e-10), tap
    # the fp32 default is what it was
    assert R.unet_forward(cfg, w, x, torch.tensor(499.0), ctx, te, ids).dtype == torch.float32


def test_chained_vae_units_are_the_oracle_decode():
    cfg = R.VAECfg(block_channels=(32, 64, 64, 64))
    w = R.make_weights(R.vae_decoder_spec(cfg), 1)
    ref, model = MU.evs(w)
    z = torch.randn(1, 4, 4, 6, generator=torch.Generator().manual_seed(4)).half()
    taps = {}
    want = R.vae_decode(cfg, ref.w, z.double() / cfg.scaling_factor, taps=taps, dtype=torch.float64)
    assert want.dtype == torch.float64
    for scaled in (True, False):
        got = _free_run(ref, cfg, MU.vae_units(cfg), lambda *a: MU.vae_unit(*a, scaled=scaled), dict(z_in=z))
        assert torch.allclose(got["image_f32"], want, rtol=0, atol=1e-11)
        for tap, unit in MU.vae_tap_names(cfg).items():
            assert torch.allclose(got[unit], taps[tap], rtol=0, atol=1e-9), tap
    # the storage model is the same function up to its roundings: close to the reference, and not equal to it
    for scaled in (True, False):
        for one in (True, False):
            m = _free_run(model, cfg, MU.vae_units(cfg), lambda *a: MU.vae_unit(*a, scaled=scaled, one_launch=one), dict(z_in=z))
            l2, _ = MU.errors(m["image_f32"], want)
            assert 0 < l2 < 1e-2, (scaled, one, l2)


def test_storage_model_of_the_unet_is_the_same_function():
    cfg = R.tiny_unet_cfg()
    w = R.make_weights(R.unet_spec(cfg), 0)
    ref, model = MU.evs(w)
    g = torch.Generator().manual_seed(5)
    B, H, W = 1, 8, 8
    inputs = dict(x_in=torch.randn(B, 4, H, W, generator=g).half(), tvals=torch.full((B,), 499.0),
                  ctx=torch.randn(B, 77, cfg.cross_dim, generator=g).half(), text_embeds=torch.randn(B, cfg.pooled_dim, generator=g).half(),
                  time_ids=torch.tensor([[128.0, 128.0, 0.0, 0.0, 128.0, 128.0]] * B))
    want = _free_run(ref, cfg, MU.unet_units(cfg), lambda *a: MU.unet_unit(*a, fused_ln=False), inputs)
    for fused in (False, True):
        got = _free_run(model, cfg, MU.unet_units(cfg), lambda *a: MU.unet_unit(*a, fused_ln=fused), inputs)
        for name in ("aug", "ctx_kv", "temb_all", "up_blocks.0.upsamplers.0.conv", "eps"):
            l2, _ = MU.errors(got[name], want[name])
            assert 0 < l2 < 1e-2, (fused, name, l2)
