"""A plain torch restatement of the TAESDXL tiny decoder (diffusers ``AutoencoderTiny`` decoder as published for
``madebyollin/taesdxl``), written from the architecture description and from nothing else - the checker of the native tiny decoder
(latentblending_amd/native/tiny_vae.py), in float64 or float32:

    x = tanh(z / 3) * 3
    decoder.layers.0                 conv 4 -> 64 (bias), ReLU
    stages with (3, 3, 3, 1) blocks  block(x) = relu(conv4(relu(conv2(relu(conv0(x))))) + x), biased 64 -> 64 convs
                                     at decoder.layers.N.conv.{0, 2, 4}
    after every stage but the last   nearest-2x upsample, conv 64 -> 64 without bias
    after the last                   conv 64 -> 3 (bias)
    image = 2 x - 1

and a generator of a state dict under the synthetic rule of the native module: W ~ N(0, gain^2 / fan_in), b ~ N(0, 0.02^2), the
last conv at gain 0.5 with 0.5 added to its three biases (frames centre on mid-grey); every value rounded to fp16, so that the
fp16 device path and this checker read bit-identical parameters.
"""
import torch
import torch.nn.functional as F

BLOCK_LAYERS = (2, 3, 4, 7, 8, 9, 12, 13, 14, 17)
UP_LAYERS = (6, 11, 16)
OUT_LAYER = 18
STAGES = ((2, 3, 4), (7, 8, 9), (12, 13, 14), (17,))       # block layers per stage; an up conv follows every stage but the last

# the keys of taesdxl's diffusion_pytorch_model.safetensors the decoder reads, in layer order
KEYS = (["decoder.layers.0.weight", "decoder.layers.0.bias"]
        + [k for n in range(2, 19) for k in (
            [f"decoder.layers.{n}.conv.{c}.{wb}" for c in (0, 2, 4) for wb in ("weight", "bias")] if n in BLOCK_LAYERS else
            [f"decoder.layers.{n}.weight"] if n in UP_LAYERS else
            [f"decoder.layers.{n}.weight", f"decoder.layers.{n}.bias"] if n == OUT_LAYER else [])])


def synthetic_state_dict(seed=0):
    """fp32 tensors holding fp16-representable values, keyed as the checkpoint."""
    g = torch.Generator().manual_seed(1000 + seed)

    def w(cout, cin, gain=1.0):
        return (torch.randn(cout, cin, 3, 3, generator=g) * gain / (cin * 9) ** 0.5).half().float()

    def b(n, shift=0.0):
        return (torch.randn(n, generator=g) * 0.02 + shift).half().float()

    sd = {"decoder.layers.0.weight": w(64, 4), "decoder.layers.0.bias": b(64)}
    for n in BLOCK_LAYERS:
        for c in (0, 2, 4):
            sd[f"decoder.layers.{n}.conv.{c}.weight"] = w(64, 64)
            sd[f"decoder.layers.{n}.conv.{c}.bias"] = b(64)
    for n in UP_LAYERS:
        sd[f"decoder.layers.{n}.weight"] = w(64, 64)
    sd[f"decoder.layers.{OUT_LAYER}.weight"] = w(3, 64, gain=0.5)
    sd[f"decoder.layers.{OUT_LAYER}.bias"] = b(3, shift=0.5)
    return sd


def decode(sd, z, dtype=torch.float64):
    """z [B, 4, H, W] (scaled latents) -> image [B, 3, 8H, 8W] in [-1, 1] (before clamping), computed in ``dtype`` on the CPU."""
    p = {k: v.detach().cpu().to(dtype) for k, v in sd.items()}

    def conv(x, name, bias=True):
        return F.conv2d(x, p[name + ".weight"], p[name + ".bias"] if bias else None, padding=1)

    x = torch.tanh(z.detach().cpu().to(dtype) / 3) * 3
    x = F.relu(conv(x, "decoder.layers.0"))
    for i, stage in enumerate(STAGES):
        for n in stage:
            h = x
            for c in (0, 2):
                h = F.relu(conv(h, f"decoder.layers.{n}.conv.{c}"))
            x = F.relu(conv(h, f"decoder.layers.{n}.conv.4") + x)
        if i < len(STAGES) - 1:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
            x = conv(x, f"decoder.layers.{UP_LAYERS[i]}", bias=False)
        else:
            x = conv(x, f"decoder.layers.{OUT_LAYER}")
    return 2 * x - 1


def to_u8(image):
    """The frame a decode stores: round_half_even(clamp(x / 2 + 0.5, 0, 1) * 255) as uint8 [B, H, W, 3]."""
    return torch.round((image / 2 + 0.5).clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
