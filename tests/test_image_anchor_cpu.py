"""Host side of image anchors (no GPU): the float64 restatement of the TAESDXL encoder and its key list, the samplers' noise
levels against the rows their step kernels read, the img2img start rule, and the engine / replay logic on the oracle's tiny CPU
pipe with a stub ``vae.encode`` and ``noise_level`` attached here."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import _taesd_enc_ref as E  # noqa: E402
from oracle import pipe as OP  # noqa: E402
from oracle import sdxl_ref as R  # noqa: E402

# ====================================================================== the restatement
# The published encoder as the issue states it: conv_in (2 keys), ten blocks of three biased convs (60), three stride-2 convs
# without bias (3), conv_out (2).  That is 67 names (a count of 68 has been quoted for this list; the layer table gives 67).
EXPECTED_KEYS = [
    "encoder.layers.0.weight", "encoder.layers.0.bias",
    "encoder.layers.1.conv.0.weight", "encoder.layers.1.conv.0.bias", "encoder.layers.1.conv.2.weight", "encoder.layers.1.conv.2.bias",
    "encoder.layers.1.conv.4.weight", "encoder.layers.1.conv.4.bias",
    "encoder.layers.2.weight",
    "encoder.layers.3.conv.0.weight", "encoder.layers.3.conv.0.bias", "encoder.layers.3.conv.2.weight", "encoder.layers.3.conv.2.bias",
    "encoder.layers.3.conv.4.weight", "encoder.layers.3.conv.4.bias",
    "encoder.layers.4.conv.0.weight", "encoder.layers.4.conv.0.bias", "encoder.layers.4.conv.2.weight", "encoder.layers.4.conv.2.bias",
    "encoder.layers.4.conv.4.weight", "encoder.layers.4.conv.4.bias",
    "encoder.layers.5.conv.0.weight", "encoder.layers.5.conv.0.bias", "encoder.layers.5.conv.2.weight", "encoder.layers.5.conv.2.bias",
    "encoder.layers.5.conv.4.weight", "encoder.layers.5.conv.4.bias",
    "encoder.layers.6.weight",
    "encoder.layers.7.conv.0.weight", "encoder.layers.7.conv.0.bias", "encoder.layers.7.conv.2.weight", "encoder.layers.7.conv.2.bias",
    "encoder.layers.7.conv.4.weight", "encoder.layers.7.conv.4.bias",
    "encoder.layers.8.conv.0.weight", "encoder.layers.8.conv.0.bias", "encoder.layers.8.conv.2.weight", "encoder.layers.8.conv.2.bias",
    "encoder.layers.8.conv.4.weight", "encoder.layers.8.conv.4.bias",
    "encoder.layers.9.conv.0.weight", "encoder.layers.9.conv.0.bias", "encoder.layers.9.conv.2.weight", "encoder.layers.9.conv.2.bias",
    "encoder.layers.9.conv.4.weight", "encoder.layers.9.conv.4.bias",
    "encoder.layers.10.weight",
    "encoder.layers.11.conv.0.weight", "encoder.layers.11.conv.0.bias", "encoder.layers.11.conv.2.weight", "encoder.layers.11.conv.2.bias",
    "encoder.layers.11.conv.4.weight", "encoder.layers.11.conv.4.bias",
    "encoder.layers.12.conv.0.weight", "encoder.layers.12.conv.0.bias", "encoder.layers.12.conv.2.weight", "encoder.layers.12.conv.2.bias",
    "encoder.layers.12.conv.4.weight", "encoder.layers.12.conv.4.bias",
    "encoder.layers.13.conv.0.weight", "encoder.layers.13.conv.0.bias", "encoder.layers.13.conv.2.weight", "encoder.layers.13.conv.2.bias",
    "encoder.layers.13.conv.4.weight", "encoder.layers.13.conv.4.bias",
    "encoder.layers.14.weight", "encoder.layers.14.bias",
]
PICTURES = [(3, 32, 32), (2, 32, 96), (1, 64, 64)]        # (B, H, W)


def test_encoder_key_list_and_shapes():
    from latentblending_amd.native import tiny_vae
    sd = E.synthetic_state_dict(0)
    assert E.KEYS == EXPECTED_KEYS == list(sd) and len(EXPECTED_KEYS) == 2 + 60 + 3 + 2
    assert "encoder.layers.2.bias" not in sd and "encoder.layers.6.bias" not in sd and "encoder.layers.10.bias" not in sd
    assert tuple(sd["encoder.layers.0.weight"].shape) == (64, 3, 3, 3)
    assert tuple(sd["encoder.layers.14.weight"].shape) == (4, 64, 3, 3) and tuple(sd["encoder.layers.14.bias"].shape) == (4,)
    for k, v in sd.items():
        if k not in ("encoder.layers.0.weight", "encoder.layers.14.weight", "encoder.layers.14.bias"):
            assert tuple(v.shape) == ((64, 64, 3, 3) if k.endswith("weight") else (64,)), k
        assert torch.equal(v, v.half().float()), f"{k}: not fp16-representable"
    assert tiny_vae.encoder_state_dict_keys() == EXPECTED_KEYS
    assert [k for k, _ in tiny_vae.encoder_layer_plan()] == ["in", "block", "down"] + ["block"] * 3 + ["down"] + ["block"] * 3 + ["down"] + ["block"] * 3 + ["out"]
    assert not set(tiny_vae.encoder_state_dict_keys()) & set(tiny_vae.state_dict_keys())


@pytest.mark.parametrize("B,H,W", PICTURES)
def test_encoder_float32_agrees_with_float64_and_latents_are_not_tiny(B, H, W):
    """34 convs of K <= 576 in float32: 1e-4 absolute (the decoder's argument); and the float64 latents have rms >= 0.05, so the
    GPU test's relative bar means something."""
    sd, u8 = E.synthetic_state_dict(0), E.pictures(B, H, W)
    z64 = E.encode(sd, u8)
    assert tuple(z64.shape) == (B, 4, H // 8, W // 8) and z64.dtype == torch.float64
    z32 = E.encode(sd, u8, dtype=torch.float32)
    err = float((z32.double() - z64).abs().max())
    rms = float(z64.pow(2).mean().sqrt())
    print(f"[enc-ref] B{B} {H}x{W}: max|f32 - f64| = {err:.3e}, rms = {rms:.4f}")
    assert err <= 1e-4
    assert rms >= 0.05


# ====================================================================== noise levels
def schedulers():
    from latentblending_amd.native import scheduler as S
    out = [(name, S.make_scheduler(name, True, "cpu")) for name in S.SCHEDULER_NAMES]
    out.append(("euler_plain", S.make_scheduler("euler", False, "cpu")))
    return out


@pytest.mark.parametrize("steps", [1, 4, 20])
def test_noise_level_reads_the_tables_of_step_row(steps):
    """Slots per include/lb_hip.h: Euler (sigma_from, sigma_next, ...); DDIM (0, sqrt(abar_t), sqrt(abar_prev), g, sqrt(1 - abar_t),
    sqrt(1 - abar_prev), 1 / sqrt(abar_t)); LCM slots 4 and 6; DPM-Solver++ (0, sigma'_i, ..., 1 / alpha_i at 6)."""
    close = lambda a, b: abs(a - b) <= 1e-6 * max(abs(a), abs(b))
    for name, s in schedulers():
        s.set_timesteps(steps)
        levels = [s.noise_level(i) for i in range(steps + 1)]
        for i in range(steps):
            a, b = levels[i]
            row = s.step_row(i)
            if s.kind == "euler":
                assert a == 1.0 and close(b, row[0]), (name, i)
                if not s.ancestral:
                    assert close(levels[i + 1][1], row[1]) or (row[1] == 0.0 and levels[i + 1][1] == 0.0), (name, i)
            elif s.kind == "ddim":
                assert close(a, row[1]) and close(b, row[4]), (name, i)
                assert close(levels[i + 1][0], row[2]) and close(levels[i + 1][1], row[5]), (name, i)
            elif s.kind == "lcm":
                assert close(a, 1.0 / row[6]) and close(b, row[4]), (name, i)
            else:
                assert s.kind == "dpmpp_2m"
                assert close(a, 1.0 / row[6]) and close(b, row[1]), (name, i)
        if s.kind == "ddim":
            a, b = levels[steps]
            assert 0.99 < a < 1.0 and 0.0 < b < 0.05, "set_alpha_to_one = False: the last step does not land on (1, 0)"
        else:
            assert levels[steps] == (1.0, 0.0), name
        bs = [b for _, b in levels]
        assert all(x > y for x, y in zip(bs, bs[1:])), (name, bs)
        for bad in (-1, steps + 1):
            with pytest.raises(ValueError):
                s.noise_level(bad)


def test_img2img_start_rule():
    from latentblending_amd import planner
    table = [(4, 0.0, 4), (4, 0.24, 4), (4, 0.25, 3), (4, 0.5, 2), (4, 0.74, 2), (4, 0.75, 1), (4, 0.99, 1), (4, 1.0, 0),
             (30, 0.3, 21), (30, 0.5, 15), (30, 1.0, 0), (30, 0.0, 30), (1, 0.5, 1), (1, 1.0, 0), (20, 0.05, 19)]
    for steps, strength, want in table:
        assert planner.img2img_start(steps, strength) == want, (steps, strength)
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError):
            planner.img2img_start(4, bad)


# ====================================================================== engine logic on the oracle's tiny CPU pipe
def stub_encode(x):
    """A VAE encoder for the tests: 8 x 8 mean of the picture in [-1, 1], the three colours and their mean as four channels."""
    assert x.ndim == 4 and x.shape[1] == 3 and float(x.min()) >= -1.0 and float(x.max()) <= 1.0
    pooled = torch.nn.functional.avg_pool2d(x.float(), 8)
    z = torch.cat([pooled, pooled.mean(1, keepdim=True)], dim=1)
    return SimpleNamespace(latent_dist=SimpleNamespace(mode=lambda: z))


def tiny_pipe(encode=True):
    p = OP.StableDiffusionXLPipeline(turbo=True, unet_cfg=R.tiny_unet_cfg(), vae_cfg=R.tiny_vae_cfg())
    p.scheduler.noise_level = lambda i: (1.0, float(p.scheduler.sigmas[i]))       # sigma space, as the native Euler samplers
    if encode:
        p.vae.encode = stub_encode
    return p


def engine(p, **kw):
    from latentblending_amd import BlendingEngine
    np.random.seed(0)
    be = BlendingEngine(p, metric=R.OracleLPIPS(7), verbose=False, **kw)
    be.set_dimensions((128, 128))
    be.set_num_inference_steps(4)
    be.set_branching(depth_strength=0.5, nmb_max_branches=3)
    be.set_prompt1("photo of a reef")
    be.set_prompt2("rendering of an alien planet")
    return be


def picture(size=(128, 128), seed=1):
    return Image.fromarray(E.pictures(1, size[1], size[0], seed)[0].numpy())


@pytest.fixture(scope="module", autouse=True)
def cpu_backend():
    """The oracle's CPU mixing backend for this module (the product's backend mixes device tensors only)."""
    from latentblending_amd.backend import set_backend
    set_backend(R.TorchCpuBackend())
    yield
    set_backend(None)


@pytest.fixture(scope="module")
def shared(cpu_backend):
    p = tiny_pipe()
    return p, engine(p)


def expected_x0(be, img):
    x = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1)[None].float() / 127.5 - 1.0
    vae = be.dh.pipe.vae                                  # (the holder hands the VAE the picture in the VAE's own dtype)
    return (stub_encode(x.to(vae.dtype)).latent_dist.mode() * vae.config.scaling_factor).half()


@pytest.mark.parametrize("strength,t_start", [(0.0, 4), (0.25, 3), (0.5, 2), (1.0, 0)])
def test_image_anchor_trajectory(shared, strength, t_start):
    p, be = shared
    be.clear_anchor_images()
    img = picture()
    be.seed1 = 77
    be.set_anchor_image1(img, strength)
    x0, eps = expected_x0(be, img), be.dh.get_unit_noise(77)
    assert torch.equal(be.dh.image2latent(img), x0)
    calls, seen = p.unet.calls, []
    inner = be.dh.run_diffusion_sd_xl

    def spy(**kw):
        seen.append(kw)
        return inner(**kw)
    be.dh.run_diffusion_sd_xl = spy
    try:
        traj = be.compute_latents_image(1)
    finally:
        del be.dh.run_diffusion_sd_xl
    assert len(traj) == 4 and all(t is not None and t.dtype == torch.float16 and tuple(t.shape) == (1, 4, 16, 16) for t in traj)
    assert be.tree_latents[0] is traj
    sig = [float(s) for s in p.scheduler.sigmas]
    for i in range(t_start):
        want = (x0.float() + sig[i + 1] * eps.float()).half() if sig[i + 1] else x0
        assert torch.equal(traj[i], want), f"entry {i}"
    assert p.unet.calls - calls == 4 - t_start
    if t_start == 4:
        assert not seen and torch.equal(traj[-1], x0), "strength 0: the anchor is the picture, no UNet evaluation"
    else:
        assert len(seen) == 1 and seen[0]["idx_start"] == t_start
        start = traj[t_start - 1] if t_start else (x0.float() + sig[0] * eps.float()).half()
        assert torch.equal(seen[0]["latents_start"], start)
        assert all(a is None for a in inner(text_embeddings=seen[0]["text_embeddings"], latents_start=start, idx_start=t_start)[:t_start])
    be.clear_anchor_images()


def test_strength_outside_the_unit_interval_raises(shared):
    _, be = shared
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="strength"):
            be.set_anchor_image1(picture(), bad)
        with pytest.raises(ValueError, match="strength"):
            be.set_anchor_image2(picture(), bad)
    assert be.anchor_image1 is None and be.anchor_image2 is None


def test_pictures_of_another_size_are_resized_at_run_time(shared):
    _, be = shared
    small = picture((200, 90), seed=3)
    be.set_anchor_image1(small, 0.0)
    traj = be.compute_latents_image(1)
    assert torch.equal(traj[-1], expected_x0(be, small.resize((128, 128), Image.LANCZOS)))
    same = picture((128, 128), seed=4)
    assert be._anchor_picture(same) is same, "a picture of the engine's size is not resampled"
    be.clear_anchor_images()


def test_a_vae_without_encode_raises():
    be = engine(tiny_pipe(encode=False))
    be.set_anchor_image1(picture(), 0.5)
    with pytest.raises(ValueError, match="no encode"):
        be.run_transition(fixed_seeds=[1, 2])


def test_a_farm_of_two_ranks_raises_before_any_work(shared):
    p, be = shared
    be.set_anchor_image2(picture(), 0.5)
    be.farm = SimpleNamespace(world=2, rank=0)
    calls = p.unet.calls
    try:
        with pytest.raises(NotImplementedError, match="farm"):
            be.run_transition(fixed_seeds=[1, 2])
    finally:
        be.farm = None
        be.clear_anchor_images()
    assert p.unet.calls == calls


def test_unit_noise_is_the_draw_of_get_noise():
    class UnitSigma(R.EulerScheduler):
        init_noise_sigma = 1.0
    p = tiny_pipe()
    be = engine(p)
    scaled = be.dh.get_noise(5)
    assert not torch.equal(scaled, be.dh.get_unit_noise(5))           # (Turbo's Euler-ancestral: sigma_max = 14.6)
    p.scheduler = UnitSigma(ancestral=True, noise_source=p.noise)
    a, b = be.dh.get_noise(5), be.dh.get_unit_noise(5)
    assert a.dtype == b.dtype == torch.float16 and a.shape == b.shape == (1, 4, 16, 16) and a.device == b.device
    assert torch.equal(a, b)


def test_run_transition_with_image_anchors_and_swap_forward(shared):
    p, be = shared
    be.clear_anchor_images()
    img1, img2 = picture(seed=5), picture(seed=6)
    be.set_anchor_image1(img1, 0.0)
    be.set_anchor_image2(img2, 0.5)
    calls = p.unet.calls
    frames = be.run_transition(fixed_seeds=[11, 12])
    assert len(frames) == 5 and len(be.tree_latents) == 5 and all(len(t) == 4 for t in (be.tree_latents[0], be.tree_latents[-1]))
    assert torch.equal(be.tree_latents[0][-1], expected_x0(be, img1))
    assert p.unet.calls - calls == 0 + 2 + 3 * 2, "anchor 1 costs nothing, anchor 2 two steps, three mid branches from step 2"
    eps2 = be.dh.get_unit_noise(12)
    want = (expected_x0(be, img2).float() + float(p.scheduler.sigmas[1]) * eps2.float()).half()
    assert torch.equal(be.tree_latents[-1][0], want)
    last = be.tree_latents[-1]
    be.swap_forward()
    assert be.anchor_image1 is img2 and be.anchor_image_strength1 == 0.5
    assert be.anchor_image2 is None and be.anchor_image_strength2 == 0.5
    # the recycled image anchor is not computed again
    be.set_prompt2("a city at night")
    calls = p.unet.calls
    be.run_transition(recycle_img1=True, fixed_seeds=[12, 13])
    assert be.tree_latents[0] is last
    assert p.unet.calls - calls == 4 + 3 * 2
    be.clear_anchor_images()
    assert (be.anchor_image1, be.anchor_image2, be.anchor_image_strength1, be.anchor_image_strength2) == (None, None, 0.5, 0.5)


def test_state_dict_keeps_its_keys_and_the_session_lists_the_fields(shared):
    from latentblending_amd import session
    _, be = shared
    keys = set(be.get_state_dict())
    be.set_anchor_image1(picture(), 0.3)
    assert set(be.get_state_dict()) == keys
    be.clear_anchor_images()
    for name in ("anchor_image1", "anchor_image2", "anchor_image_strength1", "anchor_image_strength2"):
        assert name in session._ENGINE_FIELDS and hasattr(be, name)
    assert "anchor_image1" in session._TRANSIENT_FIELDS and "anchor_image2" in session._TRANSIENT_FIELDS
    # one user's picture does not leak into another's session
    router_defaults = session._snapshot(be)
    a = session.EngineSession(be, defaults=router_defaults[:2])
    b = session.EngineSession(be, defaults=router_defaults[:2])
    with a.bound() as e:
        e.set_anchor_image1(picture(), 0.3)
    with b.bound() as e:
        assert e.anchor_image1 is None and e.anchor_image_strength1 == 0.5
    with a.bound() as e:
        assert e.anchor_image1 is not None and e.anchor_image_strength1 == 0.3
    assert be.anchor_image1 is None


def test_set_image_stubs_stay_stubs(shared):
    _, be = shared
    img = picture()
    be.set_image1(img)
    be.set_image2(img)
    assert be.image1_lowres is img and be.image2_lowres is img and be.anchor_image1 is None and be.anchor_image2 is None
    be.image1_lowres = be.image2_lowres = None


# ====================================================================== replay
def test_replay_refuses_pipelined_keyframes_with_pictures(shared):
    from latentblending_amd import replay
    _, be = shared
    with pytest.raises(ValueError, match="pipeline_keyframes"):
        replay.run_multi_transition(be, ["a", "b", "c"], [1, 2, 3], None, pipeline_keyframes=True, list_images=[None, picture(), None])
    with pytest.raises(ValueError, match="list_images"):
        replay.run_multi_transition(be, ["a", "b", "c"], [1, 2, 3], None, list_images=[None, picture()])
    with pytest.raises(ValueError, match="strength"):
        replay.run_multi_transition(be, ["a", "b"], [1, 2], None, list_images=[None, picture()], list_image_strengths=[None, 2.0])
    assert be.anchor_image1 is None and be.anchor_image2 is None


def test_replay_chain_with_a_picture_in_the_middle(shared, tmp_path):
    from latentblending_amd import replay
    p, be = shared
    be.clear_anchor_images()
    img = picture(seed=9)
    encodes = []
    inner = p.vae.encode
    p.vae.encode = lambda x: (encodes.append(1), inner(x))[1]
    try:
        p.noise.reset()
        segs = replay.run_multi_transition(be, ["a reef", "a photo", "a city"], [21, 22, 23], None,
                                           list_images=[None, img, None], list_image_strengths=[None, 0.0, None])
    finally:
        p.vae.encode = inner
    assert len(segs) == 2 and len(encodes) == 1, "the shared image key frame is encoded once and recycled"
    assert np.array_equal(np.asarray(segs[0][-1]), np.asarray(segs[1][0]))
    assert be.anchor_image1 is None and be.anchor_image2 is None, "the chain leaves no image anchor behind"
    # the same chain from a movie JSON: "image" relative to the file, "image_strength" beside it
    img.save(tmp_path / "key.png")
    items = [{"iteration": i, "seed": s, "prompt": t, "negative_prompt": ""} for i, (s, t) in
             enumerate(zip([21, 22, 23], ["a reef", "a photo", "a city"]))]
    items[1].update(image="key.png", image_strength=0.0)
    header = {"settings": "sdxl", "width": 128, "height": 128, "num_inference_steps": 4}
    with open(tmp_path / "movie.json", "w") as fh:
        json.dump([header] + items, fh)
    p.noise.reset()
    direct = replay.run_multi_transition(be, ["a reef", "a photo", "a city"], [21, 22, 23], None, list_negative_prompts=["", "", ""],
                                         list_images=[None, img, None], list_image_strengths=[None, 0.0, None])
    p.noise.reset()
    from_json = replay.run_movie_json(be, str(tmp_path / "movie.json"))
    assert len(from_json) == len(direct) == 2
    for a, b in zip(direct, from_json):
        assert len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))
