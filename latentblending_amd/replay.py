"""Multi-transition driver and the movie JSON replay format.

The reference has no function for this: the loop lives three times in its scripts
(``example_multi_trans.py:39-62``, ``example_multi_trans_json.py:24-71`` and
``latentblending/gradio_ui.py:222-262`` in /root/reference) — ``set_prompt1/2`` for the first
segment, then ``swap_forward`` + ``set_prompt2`` + ``run_transition(recycle_img1=True)`` so that every
key frame is diffused once, one movie part per segment, ``concatenate_movies`` at the end.  This module
is that loop behind two calls, with the same observable order of engine calls (so seeds, recycled
trajectories and the part files are what the scripts produce), plus reader / writer of the JSON file
the gradio UI saves (``gradio_ui.py:168-190``):

    [ {"settings": "sdxl", "width": W, "height": H, "num_inference_steps": S, "loras": [{"path": ..., "scale": ...}],
       "image_encoder": "full", "tileable": "xy"},
      {"iteration": i, "seed": s, "prompt": "...", "negative_prompt": "...", "preview_image": ...}, ... ]

``"loras"`` is optional: the LoRA adapters the whole movie is rendered under (paths relative to the JSON file).
``"image_encoder"`` is optional too: the native pipe's ``encoder`` ("tiny" / "full") the movie's image key frames are encoded with;
a file without it leaves the pipe as it stands, and ``save_movie_json`` writes the key only when it is not the default ("tiny").
``"tileable"`` is optional as well: "x" / "y" / "xy" = the movie is rendered seamless along those axes (the native pipe's
``tileable``); ``save_movie_json`` writes the key only when the setting is not off, so a default movie's file is the file it always was.
An item may also carry ``"image"`` (a picture file, path relative to the JSON file) and ``"image_strength"`` (default 0.5): that
key frame is an image anchor (``BlendingEngine.set_anchor_image1`` / ``2``) instead of a picture invented from its prompt.

Host-side control only; the hot path below it is ``BlendingEngine.run_transition``.
"""
from __future__ import annotations

import contextlib
import json
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple


def load_movie_json(fp_json: str) -> Tuple[Dict, List[Dict]]:
    """Return ``(settings, items)`` of a movie JSON (header item first, example_multi_trans_json.py:24-45)."""
    with open(fp_json, "r") as fh:
        data = json.load(fh)
    if not isinstance(data, list) or len(data) < 1 or "width" not in data[0]:
        raise ValueError(f"{fp_json}: not a latentblending movie JSON (header item with width/height missing)")
    header, items = data[0], data[1:]
    for k in ("width", "height", "num_inference_steps"):
        if k not in header:
            raise ValueError(f"{fp_json}: header lacks {k!r}")
    for it in items:
        for k in ("prompt", "negative_prompt", "seed"):
            if k not in it:
                raise ValueError(f"{fp_json}: item {it.get('iteration', '?')} lacks {k!r}")
    return header, items


def lora_entries(loras) -> List[Tuple[object, float]]:
    """``[(src, scale), ...]`` from what the drivers and the pipe's ``loras=`` accept: ``(src, scale)`` pairs, bare sources (scale 1)
    and the movie JSON's ``{"path": ..., "scale": ...}`` items."""
    out = []
    for it in loras or ():
        if isinstance(it, dict) and "path" in it:
            out.append((it["path"], float(it.get("scale", 1.0))))
        elif isinstance(it, (tuple, list)) and len(it) == 2:
            out.append((it[0], float(it[1])))
        else:
            out.append((it, 1.0))
    return out


def _loras_header(loras) -> List[Dict]:
    return [{"path": os.fspath(src), "scale": scale} for src, scale in lora_entries(loras)]


DEFAULT_IMAGE_ENCODER = "tiny"


def save_movie_json(fp_json: str, be, items: Sequence[Dict], loras: Optional[Sequence] = None,
                    image_encoder: Optional[str] = None, tileable=None) -> None:
    """Write the file the UI writes (gradio_ui.py:168-173): header from the engine's holder, then the items.  ``loras``
    (``[(path, scale), ...]``) goes into the header as ``"loras": [{"path": ..., "scale": ...}]`` - what ``run_movie_json`` loads.
    ``image_encoder``: "tiny" / "full" (None: the native pipe's ``encoder`` as it stands, "tiny" for any other pipe); written as
    ``"image_encoder"`` only when it is not the default, so a movie of the default encoder is the file it always was.
    ``tileable``: "x" / "y" / "xy" / True (None: the native pipe's ``tileable`` as it stands, off for any other pipe); written as
    ``"tileable"`` only when it is not off."""
    header = {"settings": "sdxl", "width": be.dh.width_img, "height": be.dh.height_img,
              "num_inference_steps": be.dh.num_inference_steps}
    if loras:
        header["loras"] = _loras_header(loras)
    if image_encoder is None:
        image_encoder = getattr(be.dh.pipe, "encoder", DEFAULT_IMAGE_ENCODER)
    if not isinstance(image_encoder, str) or image_encoder.strip().lower() not in ("tiny", "full"):
        raise ValueError(f"save_movie_json: image_encoder must be 'tiny' or 'full' (got {image_encoder!r})")
    if image_encoder.strip().lower() != DEFAULT_IMAGE_ENCODER:
        header["image_encoder"] = image_encoder.strip().lower()
    from .native.geometry import check_tileable         # (here: the native package imports this module)
    tileable = check_tileable(getattr(be.dh.pipe, "tileable", "") if tileable is None else tileable, "save_movie_json")
    if tileable:
        header["tileable"] = tileable
    with open(fp_json, "w") as fh:
        json.dump([header] + [dict(it) for it in items], fh, indent=4)


def run_multi_transition(be, list_prompts: Sequence[str], list_seeds: Sequence[int], fp_movie: Optional[str] = None,
                         duration_single_trans: float = 10, list_negative_prompts: Optional[Sequence[str]] = None,
                         fps: int = 30, dp_parts: str = ".", keep_parts: bool = True,
                         on_segment: Optional[Callable[[int, List], None]] = None,
                         pipeline_keyframes: bool = False, movie_encoder: Optional[str] = None,
                         movie_size=None, movie_resample: Optional[str] = None, decoder: Optional[str] = None,
                         list_images: Optional[Sequence] = None, list_image_strengths: Optional[Sequence] = None,
                         noise: Optional[str] = None, loras: Optional[Sequence] = None,
                         image_encoder: Optional[str] = None, tileable=None, control_image=None,
                         control_scale: Optional[float] = None) -> List[List]:
    """Chain ``len(list_prompts) - 1`` transitions, recycling the shared key frame of neighbouring segments.

    Engine calls are those of example_multi_trans.py:39-62; with ``list_negative_prompts`` the negative prompt
    is set as in example_multi_trans_json.py:49-58 (item ``i`` for the first segment, ``i + 1`` afterwards —
    the reference's indexing, kept).  ``fp_movie=None`` skips all file output (frames are still returned and
    handed to ``on_segment(i, frames)``).  Returns the frames of every segment.

    ``pipeline_keyframes=True`` (cross-transition pipelining): all key frames are denoised and
    decoded AHEAD of the transitions by ``BlendingEngine.precompute_keyframes`` - one lock-step batch instead of one
    latency-bound batch-1 trajectory per transition on one GPU, key frame k on rank k % world under a branch farm - and
    every transition then runs with both anchors recycled.  Prompts, negative prompts and seeds are paired exactly as
    in the sequential loop; see ``precompute_keyframes`` for the two deliberate differences (guidance scale of the key
    frames, order of ancestral noise draws).

    ``movie_encoder``: "host" / "device" for every part's ``write_movie_transition`` (None: the engine's ``movie_encoder``).
    ``movie_size`` / ``movie_resample``: its ``size_output=(W, H)`` / ``resample=`` (None: the engine's ``movie_size`` / ``movie_resample``).
    ``decoder``: "full" / "tiny" = the native pipe's ``decoder`` for this chain (None: as the pipe stands); the previous value is
    restored afterwards.
    ``list_images`` / ``list_image_strengths``: one entry per key frame, ``None`` = a prompt key frame; a picture makes that key
    frame an image anchor (``set_anchor_image1`` / ``2``; strength ``None`` = 0.5).  The image anchors are set and cleared per
    segment; a shared image key frame is computed (and encoded) once and recycled through ``swap_forward`` like any other.  The
    engine's image anchors are cleared when the chain ends.  Together with ``pipeline_keyframes=True``: ``ValueError``.
    ``noise``: "stream" / "counter" = the native pipe's ``noise`` for this chain (None: as the pipe stands); the previous value is
    restored afterwards.  Under "counter" a key frame's per-step noise depends on its seed alone, so the chain renders the same
    frames with and without ``pipeline_keyframes``, at any frontier width and under a farm of any size.
    ``loras``: ``[(src, scale), ...]`` (or the movie JSON's ``{"path": ..., "scale": ...}`` items) = LoRA adapters the native pipe
    loads for this chain (``pipe.load_lora``), once, before the first key frame, on top of what it has loaded; they are unloaded
    again afterwards.  None: the pipe's adapters as they stand.  One set per chain: a recycled key frame rendered under other
    scales would be a picture of another model.
    ``image_encoder``: "tiny" / "full" = the native pipe's ``encoder`` for this chain - what the image key frames are encoded with
    (None: as the pipe stands); the previous value is restored afterwards.
    ``tileable``: "x" / "y" / "xy" / True / False = the native pipe's ``tileable`` for this chain - seamless frames along those axes
    (None: as the pipe stands); the previous value is restored afterwards.  ``ValueError`` on a pipe without the setting.
    ``control_image`` / ``control_scale``: a ControlNet hint held through the whole chain (``BlendingEngine.set_control_image``; scale
    ``None`` = 1.0); the engine's previous hint and scale are put back afterwards.  None: the engine's hint as it stands.
    """
    images = _image_keyframes(list_images, list_image_strengths, len(list_prompts))
    if images is not None and pipeline_keyframes:
        raise ValueError("run_multi_transition: pipeline_keyframes=True precomputes every key frame from its prompt; "
                         "it cannot be combined with image key frames (list_images)")
    with _decoder_as(be, decoder), _noise_as(be, noise), _loras_as(be, loras), _encoder_as(be, image_encoder), _tileable_as(be, tileable), \
            _control_as(be, control_image, control_scale):
        try:
            return _run_multi_transition(be, list_prompts, list_seeds, fp_movie, duration_single_trans, list_negative_prompts, fps, dp_parts,
                                         keep_parts, on_segment, pipeline_keyframes, movie_encoder, movie_size, movie_resample, images)
        finally:
            if images is not None:
                be.clear_anchor_images()


def _image_keyframes(list_images, list_image_strengths, n):
    """[(picture or None, strength)] per key frame, or None when no key frame is a picture."""
    if list_images is None or all(im is None for im in list_images):
        return None
    if len(list_images) < n:
        raise ValueError("run_multi_transition needs one list_images entry (a picture or None) per prompt")
    strengths = list(list_image_strengths) if list_image_strengths is not None else [None] * len(list_images)
    if len(strengths) < n:
        raise ValueError("run_multi_transition needs one list_image_strengths entry per prompt")
    return [(im, 0.5 if s is None else float(s)) for im, s in zip(list_images[:n], strengths[:n])]


@contextlib.contextmanager
def _decoder_as(be, decoder: Optional[str]):
    """Run the body with the engine's native pipe on ``decoder`` (None: untouched), then put the previous value back."""
    if decoder is None:
        yield
        return
    pipe = be.dh.pipe
    if not hasattr(type(pipe), "decoder"):
        raise ValueError("decoder=... needs the native pipe (NativeSDXLPipe)")
    previous = pipe.decoder
    pipe.decoder = decoder
    try:
        yield
    finally:
        pipe.decoder = previous


@contextlib.contextmanager
def _encoder_as(be, encoder: Optional[str]):
    """Run the body with the engine's native pipe on ``encoder`` (None: untouched), then put the previous value back."""
    if encoder is None:
        yield
        return
    pipe = be.dh.pipe
    if not hasattr(type(pipe), "encoder"):
        raise ValueError("image_encoder=... needs the native pipe (NativeSDXLPipe)")
    previous = pipe.encoder
    pipe.encoder = encoder
    try:
        yield
    finally:
        pipe.encoder = previous


@contextlib.contextmanager
def _tileable_as(be, tileable):
    """Run the body with the engine's native pipe on ``tileable`` (None: untouched), then put the previous value back."""
    if tileable is None:
        yield
        return
    pipe = be.dh.pipe
    if not hasattr(type(pipe), "tileable"):
        raise ValueError("tileable=... needs the native pipe (NativeSDXLPipe)")
    previous = pipe.tileable
    pipe.tileable = tileable
    try:
        yield
    finally:
        pipe.tileable = previous


@contextlib.contextmanager
def _control_as(be, image, scale: Optional[float]):
    """Run the body with ``image`` as the engine's ControlNet hint (None: untouched), then put the previous hint and scale back."""
    if image is None:
        if scale is not None:
            raise ValueError("control_scale=... needs a control_image")
        yield
        return
    previous = (be.control_image, be.control_scale)
    be.set_control_image(image, 1.0 if scale is None else float(scale))
    try:
        yield
    finally:
        be.control_image, be.control_scale = previous


@contextlib.contextmanager
def _noise_as(be, noise: Optional[str]):
    """Run the body with the engine's native pipe on ``noise`` (None: untouched), then put the previous value back."""
    if noise is None:
        yield
        return
    pipe = be.dh.pipe
    if not hasattr(type(pipe), "noise"):
        raise ValueError("noise=... needs the native pipe (NativeSDXLPipe)")
    previous = pipe.noise
    pipe.noise = noise
    try:
        yield
    finally:
        pipe.noise = previous


@contextlib.contextmanager
def _loras_as(be, loras):
    """Run the body with ``loras`` loaded into the engine's native pipe on top of its own (None / empty: untouched), then unload them."""
    if not loras:
        yield
        return
    pipe = be.dh.pipe
    if not hasattr(pipe, "load_lora"):
        raise ValueError("loras=... needs the native pipe (NativeSDXLPipe)")
    names = []
    try:
        for src, scale in lora_entries(loras):
            names.append(pipe.load_lora(src, scale))
        yield
    finally:
        for name in reversed(names):
            pipe.unload_lora(name)


def _run_multi_transition(be, list_prompts, list_seeds, fp_movie, duration_single_trans, list_negative_prompts, fps, dp_parts, keep_parts,
                          on_segment, pipeline_keyframes, movie_encoder, movie_size, movie_resample, images=None) -> List[List]:
    n = len(list_prompts)
    if n < 2:
        raise ValueError("run_multi_transition needs at least two prompts")
    if len(list_seeds) < n:
        raise ValueError("run_multi_transition needs one seed per prompt")
    if list_negative_prompts is not None and len(list_negative_prompts) < n:
        raise ValueError("run_multi_transition needs one negative prompt per prompt")
    parts, segments = [], []
    keys = _precompute_chain(be, list_prompts, list_seeds, list_negative_prompts) if pipeline_keyframes else None
    for i in range(n - 1):
        if keys is not None:
            embs, trajs, key_frames = keys
            # the engine state the sequential loop would have at this point, without re-encoding anything
            be.prompt1, be.text_embedding1 = list_prompts[i].replace("_", " "), embs[i]
            be.prompt2, be.text_embedding2 = list_prompts[i + 1].replace("_", " "), embs[i + 1]
            if list_negative_prompts is not None:
                be.set_negative_prompt(list_negative_prompts[0 if i == 0 else i + 1])
            be.preset_anchors(trajs[i], trajs[i + 1], key_frames[i], key_frames[i + 1])
            frames = be.run_transition(recycle_img1=True, recycle_img2=True, fixed_seeds=[int(s) for s in list_seeds[i:i + 2]])
        elif i == 0:
            be.set_prompt1(list_prompts[i])
            if list_negative_prompts is not None:
                be.set_negative_prompt(list_negative_prompts[i])
            be.set_prompt2(list_prompts[i + 1])
            recycle_img1 = False
            if images is not None:
                be.clear_anchor_images()
                if images[0][0] is not None:
                    be.set_anchor_image1(*images[0])
        else:
            be.swap_forward()
            if list_negative_prompts is not None:
                be.set_negative_prompt(list_negative_prompts[i + 1])
            be.set_prompt2(list_prompts[i + 1])
            recycle_img1 = True
        if keys is None:
            if images is not None and images[i + 1][0] is not None:     # (swap_forward carried the previous one to anchor 1 and cleared 2)
                be.set_anchor_image2(*images[i + 1])
            fixed_seeds = [int(s) for s in list_seeds[i:i + 2]]
            frames = be.run_transition(recycle_img1=recycle_img1, fixed_seeds=fixed_seeds)
        segments.append(frames)
        if on_segment is not None:
            on_segment(i, frames)
        if fp_movie is not None:
            fp_part = os.path.join(dp_parts, f"tmp_part_{str(i).zfill(3)}.mp4")
            be.write_movie_transition(fp_part, duration_single_trans, fps=fps, encoder=movie_encoder, size_output=movie_size,
                                      resample=movie_resample)
            parts.append(fp_part)
    if fp_movie is not None:
        from .movie import concatenate_movies
        concatenate_movies(fp_movie, parts)
        if not keep_parts:
            for fp in parts:
                os.remove(fp)
    return segments


def _precompute_chain(be, list_prompts, list_seeds, list_negative_prompts):
    """Embeddings of every prompt with the negative prompt the sequential loop pairs it with (prompt 0: the engine's
    current one; prompt 1: item 0; prompt k >= 2: item k), then all key frames in one ``precompute_keyframes`` call."""
    n = len(list_prompts)
    be.set_prompt1(list_prompts[0])
    embs = [be.text_embedding1]
    for k in range(1, n):
        if list_negative_prompts is not None:
            be.set_negative_prompt(list_negative_prompts[0 if k == 1 else k])
        be.set_prompt2(list_prompts[k])
        embs.append(be.text_embedding2)
    trajs, frames = be.precompute_keyframes(embs, [int(s) for s in list_seeds[:n]])
    return embs, trajs, frames


def run_movie_json(be, fp_json: str, fp_movie: Optional[str] = None, duration_single_trans: float = 10,
                   fps: int = 30, dp_parts: str = ".", keep_parts: bool = True, pipeline_keyframes: bool = False,
                   movie_encoder: Optional[str] = None, movie_size=None, movie_resample: Optional[str] = None,
                   decoder: Optional[str] = None, noise: Optional[str] = None, loras: Optional[Sequence] = None,
                   image_encoder: Optional[str] = None, tileable=None, control_image=None,
                   control_scale: Optional[float] = None) -> List[List]:
    """``example_multi_trans_json.py`` as a call: size and step count from the header, then the chain (``decoder``, ``noise`` as there).
    Items with an ``"image"`` key (path relative to the JSON file; ``"image_strength"``, default 0.5) are image key frames.
    The header's ``"loras": [{"path": ..., "scale": ...}]`` (paths relative to the JSON file) are the chain's LoRA adapters; ``loras=``
    given here replaces them.  The header's ``"image_encoder"`` selects the encoder of the image key frames for this movie (the pipe
    is restored afterwards); ``image_encoder=`` given here replaces it; neither: the pipe as it stands.  The header's ``"tileable"``
    ("x" / "y" / "xy") renders the movie seamless along those axes, likewise; ``tileable=`` given here replaces it."""
    header, items = load_movie_json(fp_json)
    # the header's "control_image" (a path relative to the JSON file) and "control_scale": the movie's ControlNet hint;
    # control_image= / control_scale= given here replace them
    if control_image is None and header.get("control_image") is not None:
        from PIL import Image
        control_image = Image.open(os.path.join(os.path.dirname(os.path.abspath(fp_json)), header["control_image"])).convert("RGB")
    if control_scale is None and control_image is not None and header.get("control_scale") is not None:
        control_scale = float(header["control_scale"])
    if tileable is None:
        tileable = header.get("tileable")
    if image_encoder is None:
        image_encoder = header.get("image_encoder")
    if loras is None and header.get("loras"):
        base = os.path.dirname(os.path.abspath(fp_json))
        loras = [(os.path.join(base, it["path"]), float(it.get("scale", 1.0))) for it in header["loras"]]
    images = strengths = None
    if any(it.get("image") is not None for it in items):
        from PIL import Image
        base = os.path.dirname(os.path.abspath(fp_json))
        images = [None if it.get("image") is None else Image.open(os.path.join(base, it["image"])).convert("RGB") for it in items]
        strengths = [it.get("image_strength") for it in items]
    be.set_dimensions((header["width"], header["height"]))
    be.set_num_inference_steps(header["num_inference_steps"])
    return run_multi_transition(be, [it["prompt"] for it in items], [it["seed"] for it in items], fp_movie,
                                duration_single_trans, [it["negative_prompt"] for it in items], fps=fps,
                                dp_parts=dp_parts, keep_parts=keep_parts, pipeline_keyframes=pipeline_keyframes, movie_encoder=movie_encoder,
                                movie_size=movie_size, movie_resample=movie_resample, decoder=decoder, list_images=images,
                                list_image_strengths=strengths, noise=noise, loras=loras, image_encoder=image_encoder, tileable=tileable,
                                control_image=control_image, control_scale=control_scale)
