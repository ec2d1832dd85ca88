"""MI355X-native SDXL modules: UNet / VAE / LPIPS launch programs and the native pipe."""
from .pipe import NativeSDXLPipe, StableDiffusionXLPipeline
from .unet import NativeUNet, UNetConfig
from .controlnet import ControlNetConfig, NativeControlNet
from .vae import NativeVAEDecoder, NativeVAEEncoder, VAEConfig, VAEEncoderProgram, VAEProgram
from .tiny_vae import NativeTinyVAEDecoder, NativeTinyVAEEncoder, TinyEncoderProgram, TinyVAEConfig, TinyVAEProgram
from .clip import CLIPTextConfig, NativeCLIPText, NativeTextEncoders
from .weights import DictProvider, LoRAProvider, SyntheticProvider, from_safetensors, lpips_provider
from .lora import read_lora

__all__ = ["NativeSDXLPipe", "StableDiffusionXLPipeline", "NativeUNet", "UNetConfig", "NativeVAEDecoder", "NativeVAEEncoder", "VAEEncoderProgram", "VAEProgram",
           "VAEConfig", "NativeTinyVAEDecoder", "NativeTinyVAEEncoder", "TinyVAEConfig", "TinyVAEProgram", "TinyEncoderProgram", "DictProvider", "SyntheticProvider", "from_safetensors", "lpips_provider", "CLIPTextConfig", "NativeCLIPText", "NativeTextEncoders",
           "LoRAProvider", "read_lora", "ControlNetConfig", "NativeControlNet"]
