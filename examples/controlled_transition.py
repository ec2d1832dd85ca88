"""A transition guided by a ControlNet: a hint image (depth, edges, pose ...) held fixed through the whole branching tree pins the
composition of every frame, so the two prompts can differ far more before the picture starts to move.

Weights: as in single_transition.py, ``from_pretrained`` of the ``diffusers`` facade in the repository root loads the HF-layout
safetensors under ``$LB_WEIGHTS_DIR/{unet,vae,text_encoder,text_encoder_2}/``; the ControlNet is a diffusers ControlNet folder
(``config.json`` + ``*.safetensors``, e.g. a published SDXL depth or canny ControlNet) named by ``$LB_CONTROLNET_DIR``.  Without them
the pipe announces seeded synthetic stand-ins and the frames are noise-like - the script then demonstrates the calls only.  The
hint must already BE a depth map / edge map / pose drawing: hint preprocessors (Canny, depth estimation) are not part of this
project."""
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from diffusers import AutoPipelineForText2Image
from latentblending.blending_engine import BlendingEngine
from latentblending_amd.native import ControlNetConfig

pipe = AutoPipelineForText2Image.from_pretrained("stabilityai/sdxl-turbo", torch_dtype=torch.float16, variant="fp16")
pipe.to("cuda")
# a diffusers ControlNet folder - or, without one, the config that fits the UNet with seeded synthetic weights (announced)
pipe.load_controlnet(os.environ.get("LB_CONTROLNET_DIR") or ControlNetConfig.for_unet(pipe.unet_cfg))

hint_path = os.environ.get("LB_CONTROL_IMAGE")
if hint_path:
    hint = Image.open(hint_path).convert("RGB")
else:                                                       # a stand-in "depth map": a bright disc on a dark gradient
    y, x = np.mgrid[0:512, 0:512]
    disc = ((x - 256) ** 2 + (y - 300) ** 2 < 140 ** 2) * 160
    hint = Image.fromarray(np.clip(y / 8 + disc, 0, 255).astype(np.uint8)[..., None].repeat(3, axis=2))

engine = BlendingEngine(pipe, do_compile=True)
engine.set_prompt1("a marble statue in a misty forest, photo")
engine.set_prompt2("a lighthouse on a cliff at sunset, oil painting")
engine.set_control_image(hint, scale=0.8)                   # resized with LANCZOS to the render size; held for every frame
engine.run_transition(fixed_seeds=[420, 421])
engine.write_movie_transition("controlled_transition.avi", duration_transition=4)

engine.clear_control_image()                                # the uncontrolled transition of the same prompts and seeds, to compare
engine.run_transition(fixed_seeds=[420, 421])
engine.write_movie_transition("uncontrolled_transition.avi", duration_transition=4)
