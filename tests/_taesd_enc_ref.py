"""A plain torch restatement of the TAESDXL tiny ENCODER (diffusers ``AutoencoderTiny`` encoder as published for
``madebyollin/taesdxl``), written from the architecture description and from nothing else - the checker of the native tiny encoder
(latentblending_amd/native/tiny_vae.py), in float64 or float32:

    x01 = (x + 1) / 2 with x in [-1, 1]                 (a uint8 picture: u8 / 255)
    encoder.layers.0         conv 3 -> 64 (bias), no activation
    encoder.layers.1         block
    encoder.layers.2         conv 64 -> 64, stride 2, pad 1, no bias, no activation
    encoder.layers.3-5       blocks
    encoder.layers.6         stride-2 conv as above
    encoder.layers.7-9       blocks
    encoder.layers.10        stride-2 conv
    encoder.layers.11-13     blocks
    encoder.layers.14        conv 64 -> 4 (bias)
    block(x) = relu(conv4(relu(conv2(relu(conv0(x))))) + x), biased 64 -> 64 convs at encoder.layers.N.conv.{0, 2, 4}
    output = latents in scaled units (scaling_factor 1.0)

and a generator of a state dict drawn as ``_taesd_ref.synthetic_state_dict`` draws the decoder's: W ~ N(0, 1 / fan_in),
b ~ N(0, 0.02^2); every value rounded to fp16, so that the fp16 device path and this checker read bit-identical parameters.
"""
import torch
import torch.nn.functional as F

IN_LAYER = 0
BLOCK_LAYERS = (1, 3, 4, 5, 7, 8, 9, 11, 12, 13)
DOWN_LAYERS = (2, 6, 10)
OUT_LAYER = 14
STAGES = ((1,), (3, 4, 5), (7, 8, 9), (11, 12, 13))     # block layers per stage; a stride-2 conv precedes every stage but the first

# the keys of taesdxl's diffusion_pytorch_model.safetensors the encoder reads, in layer order
KEYS = [k for n in range(0, 15) for k in (
    [f"encoder.layers.{n}.conv.{c}.{wb}" for c in (0, 2, 4) for wb in ("weight", "bias")] if n in BLOCK_LAYERS else
    [f"encoder.layers.{n}.weight"] if n in DOWN_LAYERS else
    [f"encoder.layers.{n}.weight", f"encoder.layers.{n}.bias"])]


def synthetic_state_dict(seed=0):
    """fp32 tensors holding fp16-representable values, keyed as the checkpoint."""
    g = torch.Generator().manual_seed(2000 + seed)

    def w(cout, cin):
        return (torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).half().float()

    def b(n):
        return (torch.randn(n, generator=g) * 0.02).half().float()

    sd = {"encoder.layers.0.weight": w(64, 3), "encoder.layers.0.bias": b(64)}
    for n in range(1, OUT_LAYER):
        if n in BLOCK_LAYERS:
            for c in (0, 2, 4):
                sd[f"encoder.layers.{n}.conv.{c}.weight"] = w(64, 64)
                sd[f"encoder.layers.{n}.conv.{c}.bias"] = b(64)
        else:
            sd[f"encoder.layers.{n}.weight"] = w(64, 64)
    sd[f"encoder.layers.{OUT_LAYER}.weight"] = w(4, 64)
    sd[f"encoder.layers.{OUT_LAYER}.bias"] = b(4)
    return sd


def pictures(B, H, W, seed=0):
    """uint8 [B, H, W, 3]: a smooth colour field plus noise (no flat picture, no pure noise)."""
    g = torch.Generator().manual_seed(3000 + seed)
    yy = torch.linspace(0, 1, H).view(1, H, 1, 1)
    xx = torch.linspace(0, 1, W).view(1, 1, W, 1)
    phase = torch.rand(B, 1, 1, 3, generator=g) * 6.283
    freq = 1.0 + 3.0 * torch.rand(B, 1, 1, 3, generator=g)
    smooth = 0.5 + 0.35 * torch.sin(6.283 * freq * (yy + 0.6 * xx) + phase)
    x = smooth + 0.1 * torch.randn(B, H, W, 3, generator=g)
    return torch.round(x.clamp(0, 1) * 255).to(torch.uint8)


def encode(sd, u8, dtype=torch.float64):
    """uint8 pictures [B, H, W, 3] -> latents [B, 4, H / 8, W / 8] (scaled units), computed in ``dtype`` on the CPU."""
    p = {k: v.detach().cpu().to(dtype) for k, v in sd.items()}

    def conv(x, name, bias=True, stride=1):
        return F.conv2d(x, p[name + ".weight"], p[name + ".bias"] if bias else None, stride=stride, padding=1)

    x = u8.detach().cpu().to(dtype).permute(0, 3, 1, 2) / 255
    x = conv(x, f"encoder.layers.{IN_LAYER}")
    for i, stage in enumerate(STAGES):
        if i:
            x = conv(x, f"encoder.layers.{DOWN_LAYERS[i - 1]}", bias=False, stride=2)
        for n in stage:
            h = x
            for c in (0, 2):
                h = F.relu(conv(h, f"encoder.layers.{n}.conv.{c}"))
            x = F.relu(conv(h, f"encoder.layers.{n}.conv.4") + x)
    return conv(x, f"encoder.layers.{OUT_LAYER}")
