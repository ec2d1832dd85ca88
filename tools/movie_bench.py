"""Movie-part timing: ``BlendingEngine.write_movie_transition`` with the host encoder against the device encoder, same
process, same key frames, file write included; then the device path split into its stages.

    python tools/movie_bench.py [--sizes 512 1024] [--frames 300] [--keys 17] [--repeats 3] [--out profiles/movie_encode.txt]
    python tools/movie_bench.py --sizes 512 --size 1920x1080 [--resample bicubic] [--out profiles/movie_resize.txt]

With ``--size WxH`` the movie is written at that size from key frames of the ``--sizes`` render size (``size_output=``): the host
path of the same commit (Pillow resize + host in-betweening + host encode) against the device path, the device path's stages, and
the resample launches alone against their traffic floor and the copy bandwidth this run reaches.

The key frames are 17 synthetic device-resident frames (smooth gradients + Gaussian noise, sigma 6: about the byte count of a
render at quality 92), handed to the engine's own methods through a stand-in that carries only what those methods read
(``tree_final_imgs``, the render size, ``movie_encoder``) - no model is loaded.  JPEG time depends on content: a real render
moves the figures by its byte count, not the comparison.
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import time
import types
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from latentblending_amd.blending_engine import BlendingEngine  # noqa: E402
from latentblending_amd.hip import ops  # noqa: E402
from latentblending_amd.jpeg import EOI, jpeg_header  # noqa: E402
from latentblending_amd.movie import AviMovieSaver  # noqa: E402
from latentblending_amd.native.frames import DeviceImage  # noqa: E402
from latentblending_amd.utils import inbetween_frames_device, resize_frames_device  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, MI355X


class EngineStandIn:
    """What ``write_movie_transition`` reads of an engine, around the engine's own (unmodified) methods."""
    write_movie_transition = BlendingEngine.write_movie_transition
    _write_movie_transition_device = BlendingEngine._write_movie_transition_device
    _movie_output = BlendingEngine._movie_output
    verbose = False
    movie_encoder = "host"
    movie_size = None
    movie_resample = "bicubic"

    def __init__(self, frames, size):
        self.tree_final_imgs = frames
        self.dh = types.SimpleNamespace(height_img=size, width_img=size)


def key_frames(size, n_keys, device):
    g = torch.Generator(device="cpu").manual_seed(0)
    y, x = torch.meshgrid(torch.arange(size, dtype=torch.float32), torch.arange(size, dtype=torch.float32), indexing="ij")
    out = []
    for k in range(n_keys):
        base = torch.stack([40 + 170 * x / (size - 1), 30 + 190 * y / (size - 1),
                            128 + 90 * torch.sin(x / 37.0 + k) * torch.cos(y / 23.0 + 0.3 * k)], dim=-1)
        frame = (base + 6.0 * torch.randn(base.shape, generator=g)).round().clamp(0, 255).to(torch.uint8)
        out.append(DeviceImage(frame.to(device)))
    return out


def timed(fn, repeats):
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return min(times), float(np.median(times))


def stage_split(frames_keys, size, n_frames, fp, repeats):
    """Median milliseconds of the device path's stages, run one after the other with a synchronisation between them."""
    code, h, w = 0, size, size
    res = {}
    np.random.seed(0)
    blended = inbetween_frames_device(frames_keys, n_frames)

    def lerp():
        np.random.seed(0)
        inbetween_frames_device(frames_keys, n_frames)
    res["lerp (frames_lerp_u8 + cat)"] = timed(lerp, repeats)[1]
    dev = blended.device
    qt = ops._jpeg_qtables(92, dev)
    chunk = max(1, min(blended.shape[0], 1024, ops._JPEG_WORKSPACE_BUDGET // ops.api.lb_jpeg_workspace_bytes(1, h, w, code)))
    header = jpeg_header(h, w, 92, "4:2:0")
    files, traffic, total = [], 0, 0
    names = ("stage 1 (colour + DCT + quantise)", "stage 2 + scan + compaction", "copy (sizes, then payload through the pinned buffer)",
             "per-frame bytes objects (header + scan + EOI)")
    for name in names:
        res[name] = 0.0
    for k0 in range(0, blended.shape[0], chunk):                      # the chunks of ops.jpeg_encode_u8, stage by stage
        part = blended[k0:k0 + chunk]
        n = part.shape[0]
        coef = torch.empty(ops.api.lb_jpeg_coefficient_count(n, h, w, code), dtype=torch.int16, device=dev)
        ws = torch.empty(ops.api.lb_jpeg_workspace_bytes(n, h, w, code), dtype=torch.uint8, device=dev)
        out = torch.empty(n * (h * w + 4096), dtype=torch.uint8, device=dev)
        fb = torch.empty(n, dtype=torch.int32, device=dev)
        res[names[0]] += timed(lambda: ops.jpeg_dct_quant_into(part, qt, coef, code), repeats + 2)[0]
        traffic += part.numel() + coef.numel() * 2
        res[names[1]] += timed(lambda: ops.jpeg_entropy_into(coef, ws, out, fb, n, h, w, code), repeats + 2)[0]
        sizes = fb.cpu().tolist()
        nbytes = sum(sizes)
        total += nbytes

        def copy():
            fb.cpu()
            ops._jpeg_to_host(out, nbytes)
        res[names[2]] += timed(copy, repeats)[1]
        host = ops._jpeg_to_host(out, nbytes)

        def split():
            made, pos = [], 0
            for s in sizes:
                made.append(b"".join((header, bytes(host[pos:pos + s]), EOI)))
                pos += s
            return made
        res[names[3]] += timed(split, repeats)[1]
        files.extend(split())
        del coef, ws, out
    s1 = res[names[0]]
    res["_stage1_note"] = f"stage 1 moves {traffic / 1e6:.1f} MB in {s1 * 1e3:.3f} ms = {traffic / s1 / 1e12:.2f} TB/s = " \
                          f"{100 * traffic / s1 / HBM_PEAK:.0f} % of the 8 TB/s HBM peak ({-(-blended.shape[0] // chunk)} chunk(s) of <= {chunk} frames)"

    def container():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            saver = AviMovieSaver(fp, fps=30, shape_hw=[h, w])
        saver._jpegs.extend(files)
        saver.finalize()
    res["container (AVI assembly + file write)"] = timed(container, repeats)[1]
    res["_bytes"] = total
    return res


def event_ms(fn, iters):
    """Mean milliseconds of ``fn`` over ``iters`` back-to-back calls between two device events (after one warm-up call)."""
    fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def resize_rows(size, out_wh, filt, args):
    """Lines for one movie part of ``out_wh`` = (W, H) from ``size`` x ``size`` key frames."""
    w, h = out_wh
    duration, fps = args.frames / 30.0, 30
    lines = []
    with tempfile.TemporaryDirectory() as td:
        frames = key_frames(size, args.keys, "cuda")
        eng = EngineStandIn(frames, size)
        row = {}
        for enc in ("host", "device"):
            fp = os.path.join(td, f"{enc}.avi")

            def run(enc=enc, fp=fp):
                np.random.seed(0)
                eng.write_movie_transition(fp, duration, fps=fps, encoder=enc, size_output=(w, h), resample=filt)
            run()
            row[enc] = timed(run, args.repeats) + (os.path.getsize(fp),)
        from latentblending_amd.movie import read_movie_header, read_movie_jpegs
        import io
        from PIL import Image
        jpegs = read_movie_jpegs(os.path.join(td, "device.avi"))
        decoded = [Image.open(io.BytesIO(jpegs[k])) for k in (0, len(jpegs) // 2, -1)]
        for im in decoded:
            im.load()
        playable = f"device file: (fps, H, W, frames) = {read_movie_header(os.path.join(td, 'device.avi'))}, frames 0 / middle / last decode to {[im.size for im in decoded]}"
        tag = f"{size}x{size} -> {w}x{h} {filt}"
        lines.append(f"{tag}: host   {row['host'][0] * 1e3:8.1f} / {row['host'][1] * 1e3:8.1f} ms   ({row['host'][2] / 1e6:.1f} MB file)")
        lines.append(f"{tag}: device {row['device'][0] * 1e3:8.1f} / {row['device'][1] * 1e3:8.1f} ms   ({row['device'][2] / 1e6:.1f} MB file)"
                     f"   host / device = {row['host'][1] / row['device'][1]:.1f}x")
        lines.append(f"    {playable}")
        # the device path stage by stage (median, a synchronisation after each)
        keys = resize_frames_device(frames, (h, w), filt)
        np.random.seed(0)
        blended = inbetween_frames_device(keys, args.frames)
        split = {"resize (stack the key frames + ops.resample_u8)": timed(lambda: resize_frames_device(frames, (h, w), filt), args.repeats + 2)[1]}

        def lerp():
            np.random.seed(0)
            inbetween_frames_device(keys, args.frames)
        split["in-between (frames_lerp_u8 + cat)"] = timed(lerp, args.repeats + 2)[1]
        try:
            files = ops.jpeg_encode_u8(blended)
            split["encode (ops.jpeg_encode_u8, compressed bytes to the host)"] = timed(lambda: ops.jpeg_encode_u8(blended), args.repeats)[1]
        except RuntimeError:                                           # a size the encoder does not take: the writer's host fall-back
            def host_encode():
                saver = AviMovieSaver(os.path.join(td, "x.avi"), fps=fps, shape_hw=[h, w])
                for frame in blended.cpu().numpy():
                    saver.write_frame(frame)
                return saver._jpegs
            files = host_encode()
            split["encode (host fall-back: raw frames to the host, Pillow)"] = timed(host_encode, 1)[1]

        def container():
            saver = AviMovieSaver(os.path.join(td, "c.avi"), fps=fps, shape_hw=[h, w])
            saver._jpegs.extend(files)
            saver.finalize()
        split["file write (AVI assembly + write)"] = timed(container, args.repeats)[1]
        for name, v in split.items():
            lines.append(f"    {name:<62s} {v * 1e3:9.3f} ms")
        # the launcher alone on the stacked key frames, against its traffic floor and a device-to-device copy of this run
        stack = torch.stack([f._lb_u8 for f in frames])
        n = stack.shape[0]
        tx, ty = ops._resample_tables(size, size, h, w, filt, stack.device)
        tmp = torch.empty((n, size, w, 3), dtype=torch.uint8, device=stack.device)
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=stack.device)
        ms = event_ms(lambda: ops.resample_u8_into(stack, tmp if tx is not None and ty is not None else None, out, tx, ty), 50)
        same = torch.equal(out, keys)
        floor = n * 3 * (size * size + 2 * size * w + h * w)
        big = torch.empty(1 << 29, dtype=torch.uint8, device=stack.device)
        dst = torch.empty_like(big)
        copy_ms = event_ms(lambda: dst.copy_(big), 10)
        copy_bw = 2 * big.numel() / (copy_ms * 1e-3)
        lines.append(f"    lb_resample_u8 alone, {n} key frames: {ms * 1e3:.1f} us for a floor of {floor / 1e6:.1f} MB = {floor / (ms * 1e-3) / 1e12:.2f} TB/s = "
                     f"{100 * floor / (ms * 1e-3) / copy_bw:.0f} % of the {copy_bw / 1e12:.2f} TB/s a 512 MiB device-to-device copy reaches in this run "
                     f"({100 * copy_bw / HBM_PEAK:.0f} % of the 8 TB/s HBM peak)")
        for name, fn, nbytes in (("horizontal pass alone", lambda: ops.resample_u8_into(stack, None, tmp, tx, None), n * 3 * (size * size + size * w)),
                                 ("vertical pass alone", lambda: ops.resample_u8_into(tmp, None, out, None, ty), n * 3 * (size * w + h * w))):
            if (tx if name.startswith("h") else ty) is not None:
                ms = event_ms(fn, 50)
                lines.append(f"        {name}: {ms * 1e3:.1f} us for {nbytes / 1e6:.1f} MB = {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s = "
                             f"{100 * nbytes / (ms * 1e-3) / copy_bw:.0f} % of the copy")
        lines.append(f"    launcher output equals resize_frames_device: {same}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--keys", type=int, default=17)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", action="append", default=[], metavar="WxH", help="write the movie at this size (may be repeated)")
    ap.add_argument("--resample", default="bicubic")
    args = ap.parse_args()
    if args.size:
        lines = [f"# tools/movie_bench.py --size: one movie part of {args.frames} frames from {args.keys} key frames, resized with size_output=, "
                 f"quality 92, 4:2:0, {torch.cuda.get_device_name(0)}",
                 f"# write_movie_transition, wall clock with the file write, after one warm-up call each; min / median of {args.repeats} runs"]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for size in args.sizes:
                for spec in args.size:
                    w, h = (int(v) for v in spec.lower().split("x"))
                    lines += resize_rows(size, (w, h), args.resample, args)
        text = "\n".join(lines)
        print(text, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(text + "\n")
        return
    duration, fps = args.frames / 30.0, 30
    lines = [f"# tools/movie_bench.py: one movie part of {args.frames} frames from {args.keys} key frames, quality 92, 4:2:0, {torch.cuda.get_device_name(0)}",
             "# write_movie_transition, wall clock with the file write, after one warm-up call each; min / median of "
             f"{args.repeats} runs"]
    with tempfile.TemporaryDirectory() as td, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for size in args.sizes:
            frames = key_frames(size, args.keys, "cuda")
            eng = EngineStandIn(frames, size)
            row = {}
            for enc in ("host", "device"):
                fp = os.path.join(td, f"{enc}_{size}.avi")

                def run(enc=enc, fp=fp):
                    np.random.seed(0)
                    eng.write_movie_transition(fp, duration, fps=fps, encoder=enc)
                run()
                row[enc] = timed(run, args.repeats) + (os.path.getsize(fp),)
            lines.append(f"{size}x{size}: host   {row['host'][0] * 1e3:8.1f} / {row['host'][1] * 1e3:8.1f} ms   ({row['host'][2] / 1e6:.1f} MB file)")
            lines.append(f"{size}x{size}: device {row['device'][0] * 1e3:8.1f} / {row['device'][1] * 1e3:8.1f} ms   ({row['device'][2] / 1e6:.1f} MB file)"
                         f"   host / device = {row['host'][1] / row['device'][1]:.1f}x")
            split = stage_split(frames, size, args.frames, os.path.join(td, f"split_{size}.avi"), args.repeats)
            for name, v in split.items():
                if not name.startswith("_"):
                    lines.append(f"    {name:<55s} {v * 1e3:9.3f} ms")
            lines.append(f"    {split['_stage1_note']}")
            lines.append(f"    scan data: {split['_bytes'] / 1e6:.1f} MB across the bus instead of {args.frames * size * size * 3 / 1e6:.0f} MB of raw frames")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
