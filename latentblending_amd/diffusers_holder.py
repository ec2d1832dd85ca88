"""``DiffusersHolder`` — the diffusion runner behind the blending engine.

Same public surface as the reference class (``latentblending/diffusers_holder.py:20-366`` in
/root/reference): constructor, ``set_num_inference_steps``, ``set_dimensions``,
``set_negative_prompt``, ``get_text_embedding``, ``get_noise``, ``latent2image``,
``prepare_mixing``, ``run_diffusion`` and ``run_diffusion_sd_xl`` with identical argument
order, defaults and return types.

Two execution paths behind that surface:

* **native** — the pipe is a ``NativeSDXLPipe`` (``pipe.is_lb_native``): the restartable
  denoising loop (skip ``i < idx_start``, crossfeed slerp, scale, UNet, CFG, Euler step) runs as
  hand-written gfx950 kernels on device-resident state; this module only forwards arguments.
* **generic** — any object with the SDXL pipeline duck type, e.g. a real
  diffusers ``StableDiffusionXLPipeline`` or the CPU oracle pipe in ``oracle/``.  The loop below
  drives ``pipe.unet`` / ``pipe.scheduler`` step by step exactly like the reference and takes the
  crossfeed slerp from the active mixing backend.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .backend import get_backend


def _is_native(pipe) -> bool:
    return bool(getattr(pipe, "is_lb_native", False))


class DiffusersHolder:
    def __init__(self, pipe):
        self.negative_prompt = ""
        self.guidance_scale = 5.0
        self.num_inference_steps = 30

        self.pipe = pipe
        self.device = str(pipe._execution_device)
        self.init_types()

        latent_side = self.pipe.unet.config.sample_size
        self.width_latent = latent_side
        self.height_latent = latent_side
        self.width_img = latent_side * self.pipe.vae_scale_factor
        self.height_img = latent_side * self.pipe.vae_scale_factor
        # ControlNet hint (set_control): the picture as given, and what the generic loop feeds pipe.controlnet
        self.control_image = None
        self.control_scale = 1.0
        self._control_token = None
        self._control_cond = None

    # ---------------------------------------------------------------- configuration -------
    def init_types(self):
        cls = getattr(self.pipe, "__class__", None)
        assert cls is not None and hasattr(cls, "__name__"), "No valid diffusers pipeline found."
        if cls.__name__ == 'StableDiffusionXLPipeline':
            self.pipe.scheduler.set_timesteps(self.num_inference_steps, device=self.device)
            probe = self.pipe.encode_prompt("test")[0]
        else:
            probe = self.pipe._encode_prompt("test", self.device, 1, True)
        self.dtype = probe.dtype
        self.is_sdxl_turbo = 'turbo' in self.pipe._name_or_path

    def set_num_inference_steps(self, num_inference_steps):
        self.num_inference_steps = num_inference_steps
        self.pipe.scheduler.set_timesteps(self.num_inference_steps, device=self.device)

    def set_dimensions(self, size_output):
        """``size_output`` = (width, height); snapped to a multiple of the VAE scale factor."""
        scale = self.pipe.vae_scale_factor
        if size_output is None:
            width = height = self.pipe.unet.config.sample_size
        else:
            width, height = size_output
        self.width_img = int(round(width / scale) * scale)
        self.width_latent = int(self.width_img / scale)
        self.height_img = int(round(height / scale) * scale)
        self.height_latent = int(self.height_img / scale)
        print(f"set_dimensions to width={width} and height={height}")

    def set_negative_prompt(self, negative_prompt):
        """Only one negative prompt is supported: a string or the first entry of a list."""
        as_list = [negative_prompt] if isinstance(negative_prompt, str) else negative_prompt
        self.negative_prompt = as_list[:1] if len(as_list) > 1 else as_list

    def set_control(self, image, scale: float = 1.0):
        """Hold ``image`` (a PIL image or uint8 [H, W, 3]; None: no control) as the ControlNet hint of every UNet evaluation, at
        conditioning scale ``scale``.  Native pipe: ``pipe.set_control_image`` / ``clear_control`` (the controlled launch programs).
        Any other pipe: the generic loop calls ``pipe.controlnet(...)`` the way diffusers' ControlNet pipeline does - the picture
        resized with LANCZOS to the holder's size, float in [0, 1] (not normalised to +-1), the same hint for both CFG halves.
        Calling it again with the same picture, scale and size does nothing."""
        token = None if image is None else (id(image), float(scale), self.width_img, self.height_img)
        if token == self._control_token and (image is None or image is self.control_image):
            return
        pipe = self.pipe
        if image is not None and not (callable(getattr(pipe, "controlnet", None)) or hasattr(pipe, "set_control_image")):
            raise ValueError(f"set_control: the pipe ({type(pipe).__name__}) has no controlnet")
        if _is_native(pipe):        # the controlled launch programs (the generic loop below, on a native pipe, goes through its facades)
            if image is None:
                if hasattr(pipe, "clear_control"):
                    pipe.clear_control()
            else:
                pipe.set_control_image(image, float(scale))
        if image is not None:
            from PIL import Image
            pic = image.convert("RGB") if isinstance(image, Image.Image) else None
            if pic is None:
                arr = np.asarray(image)
                if arr.ndim != 3 or arr.shape[-1] != 3 or arr.dtype != np.uint8:
                    raise ValueError(f"control image: expected a PIL image or a uint8 [H, W, 3] picture (got {arr.dtype} {arr.shape})")
                pic = Image.fromarray(arr)
            if pic.size != (self.width_img, self.height_img):
                pic = pic.resize((self.width_img, self.height_img), Image.LANCZOS)
            u8 = torch.from_numpy(np.asarray(pic, dtype=np.uint8).copy())
            self._control_cond = (u8.permute(2, 0, 1)[None].to(torch.float32) / 255.0).to(pipe._execution_device)
        if image is None:
            self._control_cond = None
        self.control_image, self.control_scale, self._control_token = image, float(scale), token

    # ---------------------------------------------------------------- pipeline helpers ----
    def get_text_embedding(self, prompt):
        """4-tuple (prompt_embeds, negative_prompt_embeds, pooled, negative_pooled)."""
        wants_cfg = self.guidance_scale > 1 and self.pipe.unet.config.time_cond_proj_dim is None
        return self.pipe.encode_prompt(
            prompt=prompt, prompt_2=prompt, device=self.pipe._execution_device,
            num_images_per_prompt=1, do_classifier_free_guidance=wants_cfg,
            negative_prompt=self.negative_prompt, negative_prompt_2=self.negative_prompt,
            prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None,
            negative_pooled_prompt_embeds=None, lora_scale=None, clip_skip=None)

    def get_noise(self, seed=420):
        """Initial latent for ``seed``: always fp16, scaled by the scheduler's init sigma
        (the reference hard-codes float16 here, ``diffusers_holder.py:105``)."""
        generator = torch.Generator(device=self.device).manual_seed(int(seed))
        return self.pipe.prepare_latents(
            1, self.pipe.unet.config.in_channels, self.height_img, self.width_img,
            torch.float16, self.pipe._execution_device, generator, None)

    def get_unit_noise(self, seed=420):
        """The tensor ``get_noise(seed)`` draws - same generator, shape, dtype and device - WITHOUT the multiplication by the
        scheduler's ``init_noise_sigma``: the ``eps`` of a forward-noised picture (``a x0 + b eps``, image anchors)."""
        generator = torch.Generator(device=self.device).manual_seed(int(seed))
        pipe = self.pipe
        if _is_native(pipe):
            return pipe.unit_noise(1, pipe.unet.config.in_channels, self.height_img, self.width_img, torch.float16,
                                   pipe._execution_device, generator)
        # a diffusers-like pipe: its prepare_latents is randn_tensor(...) * init_noise_sigma and offers the draw in no other way, so
        # the sigma is divided out again (nothing to do when it is 1; otherwise within one fp16 rounding of the draw)
        sigma = float(getattr(pipe.scheduler, "init_noise_sigma", 1.0))
        z = pipe.prepare_latents(1, pipe.unet.config.in_channels, self.height_img, self.width_img, torch.float16,
                                 pipe._execution_device, generator, None)
        return z if sigma == 1.0 else (z.float() / sigma).to(z.dtype)

    @torch.no_grad()
    def image2latent(self, image) -> torch.Tensor:
        """Encode a picture (PIL image, or what the pipe's encoder takes) of the holder's size to scaled latents [1, 4, h, w]:
        the native pipe's ``native_image2latent`` (its ``encoder``: TAESDXL, or the full SDXL VAE encoder), else ``pipe.vae.encode`` of the picture in [-1, 1] (``latent_dist.mode()`` when the
        VAE returns a distribution, else ``.latents``) times ``vae.config.scaling_factor``."""
        pipe = self.pipe
        if _is_native(pipe):
            pipe.render_size = (self.height_img, self.width_img)
            return pipe.native_image2latent(image)
        vae = pipe.vae
        if not callable(getattr(vae, "encode", None)):
            raise ValueError(f"image2latent: the pipe's VAE ({type(vae).__name__}) has no encode(); an image anchor needs an encoder")
        u8 = np.asarray(image.convert("RGB") if hasattr(image, "convert") else image, dtype=np.uint8)
        if u8.shape[:2] != (self.height_img, self.width_img):
            raise ValueError(f"image2latent: the picture is {u8.shape[1]} x {u8.shape[0]} (width x height) but the holder renders "
                             f"{self.width_img} x {self.height_img}")
        x = torch.from_numpy(u8.copy()).permute(2, 0, 1)[None].to(device=pipe._execution_device, dtype=torch.float32) / 127.5 - 1.0
        out = vae.encode(x.to(getattr(vae, "dtype", x.dtype)))
        dist = getattr(out, "latent_dist", None)
        z = dist.mode() if dist is not None else out.latents
        return (z * vae.config.scaling_factor).to(torch.float16)

    @torch.no_grad()
    def latent2image(self, latents: torch.Tensor, output_type="pil"):
        """Decode a final latent to an image ("pil" or "np")."""
        assert output_type in ["pil", "np"]
        if _is_native(self.pipe):
            return self.pipe.native_latent2image(latents, output_type)

        vae = self.pipe.vae
        upcast = vae.dtype == torch.float16 and vae.config.force_upcast
        if upcast:
            self.pipe.upcast_vae()
            latents = latents.to(next(iter(vae.post_quant_conv.parameters())).dtype)
        image = vae.decode(latents / vae.config.scaling_factor, return_dict=False)[0]
        if upcast:
            vae.to(dtype=torch.float16)
        return self.pipe.image_processor.postprocess(image, output_type=output_type)[0]

    def prepare_mixing(self, mixing_coeffs, list_latents_mixing):
        steps = self.num_inference_steps
        if type(mixing_coeffs) == float:
            coeffs = (1 + steps) * [mixing_coeffs]
        elif type(mixing_coeffs) == list:
            assert len(mixing_coeffs) == steps, \
                f"len(mixing_coeffs) {len(mixing_coeffs)} != self.num_inference_steps {steps}"
            coeffs = mixing_coeffs
        else:
            raise ValueError("mixing_coeffs should be float or list with len=num_inference_steps")
        if np.sum(coeffs) > 0:
            assert len(list_latents_mixing) == steps, \
                f"len(list_latents_mixing) {len(list_latents_mixing)} != self.num_inference_steps {steps}"
        return coeffs

    # ---------------------------------------------------------------- diffusion -----------
    @torch.no_grad()
    def run_diffusion(self, text_embeddings, latents_start, idx_start: int = 0,
                      list_latents_mixing=None, mixing_coeffs=0.0,
                      return_image: Optional[bool] = False):
        return self.run_diffusion_sd_xl(text_embeddings, latents_start, idx_start,
                                        list_latents_mixing, mixing_coeffs, return_image)

    @torch.no_grad()
    def run_diffusion_sd_xl(self, text_embeddings: tuple, latents_start: torch.Tensor,
                            idx_start: int = 0, list_latents_mixing=None, mixing_coeffs=0.0,
                            return_image: Optional[bool] = False):
        """Denoise from step ``idx_start``; returns a list with one entry per step (``None`` for
        skipped steps, otherwise the latent after that step) or the decoded image."""
        coeffs = self.prepare_mixing(mixing_coeffs, list_latents_mixing)
        if _is_native(self.pipe):
            trajectory = self.pipe.native_run_diffusion(
                text_embeddings, latents_start, idx_start, list_latents_mixing, coeffs,
                num_inference_steps=self.num_inference_steps, guidance_scale=self.guidance_scale)
        else:
            trajectory = self._denoise_generic(text_embeddings, latents_start, idx_start,
                                               list_latents_mixing, coeffs)
        if return_image:
            return self.latent2image(trajectory[-1])
        return trajectory

    # generic duck-typed pipe ---------------------------------------------------------------
    def _conditioning_generic(self, text_embeddings):
        pipe = self.pipe
        prompt_embeds, neg_prompt_embeds, pooled, neg_pooled = text_embeddings
        # The micro-conditioning always describes the UNet's native size, not the render size
        # (reference quirk, diffusers_holder.py:216-220).
        side = pipe.default_sample_size * pipe.vae_scale_factor
        if pipe.text_encoder_2 is None:
            proj_dim = int(pooled.shape[-1])
        else:
            proj_dim = pipe.text_encoder_2.config.projection_dim
        time_ids = pipe._get_add_time_ids((side, side), (0, 0), (side, side),
                                          dtype=prompt_embeds.dtype,
                                          text_encoder_projection_dim=proj_dim)
        text_embeds = pooled
        if pipe.do_classifier_free_guidance:
            prompt_embeds = torch.cat([neg_prompt_embeds, prompt_embeds], dim=0)
            text_embeds = torch.cat([neg_pooled, text_embeds], dim=0)
            time_ids = torch.cat([time_ids, time_ids], dim=0)
        device = pipe._execution_device
        return prompt_embeds.to(device), text_embeds.to(device), time_ids.to(device).repeat(1, 1)

    def _denoise_generic(self, text_embeddings, latents_start, idx_start, list_latents_mixing,
                         coeffs):
        pipe = self.pipe
        slerp = get_backend().slerp

        pipe._guidance_scale = self.guidance_scale
        pipe._guidance_rescale = 0.0
        pipe._clip_skip = None
        pipe._cross_attention_kwargs = None
        pipe._denoising_end = None
        pipe._interrupt = False

        device = pipe._execution_device
        pipe.scheduler.set_timesteps(self.num_inference_steps, device=device)
        timesteps = pipe.scheduler.timesteps
        step_kwargs = pipe.prepare_extra_step_kwargs(None, 0.0)
        prompt_embeds, text_embeds, time_ids = self._conditioning_generic(text_embeddings)

        latents = latents_start.clone()
        timestep_cond = None
        if pipe.unet.config.time_cond_proj_dim is not None:
            w = torch.tensor(pipe.guidance_scale - 1).repeat(1)
            timestep_cond = pipe.get_guidance_scale_embedding(
                w, embedding_dim=pipe.unet.config.time_cond_proj_dim
            ).to(device=device, dtype=latents.dtype)
        pipe._num_timesteps = len(timesteps)

        trajectory = []
        for i, t in enumerate(timesteps):
            if i < idx_start:
                trajectory.append(None)
                continue
            if i == idx_start:
                latents = latents_start.clone()
            if i > 0 and coeffs[i] > 0:
                latents = slerp(latents, list_latents_mixing[i - 1].clone(), coeffs[i])

            cfg = pipe.do_classifier_free_guidance
            model_in = torch.cat([latents] * 2) if cfg else latents
            model_in = pipe.scheduler.scale_model_input(model_in, t)
            added = {"text_embeds": text_embeds, "time_ids": time_ids}
            control = {}
            if self._control_cond is not None:      # diffusers' ControlNet pipeline: the ControlNet sees the UNet's own inputs
                cond = self._control_cond.to(model_in.dtype)
                down, mid = pipe.controlnet(
                    model_in, t, encoder_hidden_states=prompt_embeds, controlnet_cond=torch.cat([cond] * 2) if cfg else cond,
                    conditioning_scale=self.control_scale, added_cond_kwargs=added, return_dict=False)
                control = {"down_block_additional_residuals": down, "mid_block_additional_residual": mid}
            eps = pipe.unet(
                model_in, t, encoder_hidden_states=prompt_embeds, timestep_cond=timestep_cond,
                cross_attention_kwargs=pipe.cross_attention_kwargs,
                added_cond_kwargs=added, return_dict=False, **control)[0]
            if cfg:
                eps_uncond, eps_text = eps.chunk(2)
                eps = eps_uncond + pipe.guidance_scale * (eps_text - eps_uncond)
            latents = pipe.scheduler.step(eps, t, latents, **step_kwargs, return_dict=False)[0]
            trajectory.append(latents.clone())
        return trajectory
