"""A transition whose frames tile: every conv of the UNet and the decoder pads by wrap-around (``tileable="xy"``), so the left edge
of a frame meets its right edge and the top meets the bottom.  Writes the first frame as a 2 x 2 mosaic for looking at the seams.

Weights: as in single_transition.py, ``from_pretrained`` of the ``diffusers`` facade in the repository root loads the HF-layout
safetensors under ``$LB_WEIGHTS_DIR/{unet,vae,text_encoder,text_encoder_2}/``; without them the pipe announces seeded synthetic
stand-ins and the frames are noise-like - the script then demonstrates the calls only.  ``tileable`` is a setting of the native
pipe: ``NativeSDXLPipe(tileable="xy", unet_provider=native.from_safetensors(<dir>/unet), ...)`` sets it at construction."""
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from diffusers import AutoPipelineForText2Image
from latentblending.blending_engine import BlendingEngine
from latentblending_amd.utils import tile_preview

pipe = AutoPipelineForText2Image.from_pretrained("stabilityai/sdxl-turbo", torch_dtype=torch.float16, variant="fp16")
pipe.to("cuda")
pipe.tileable = "xy"                                    # "x": a 360 degree strip; "xy": a tileable texture; None: off
engine = BlendingEngine(pipe, do_compile=True)
engine.set_prompt1("mossy cobblestones, top-down texture")
engine.set_prompt2("cracked desert clay, top-down texture")
frames = engine.run_transition(fixed_seeds=[420, 421])
Image.fromarray(tile_preview(np.asarray(frames[0]), nx=2, ny=2)).save("tileable_mosaic.png")
engine.write_movie_transition("tileable_transition.avi", duration_transition=4)
