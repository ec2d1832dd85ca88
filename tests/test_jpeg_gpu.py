"""Device MJPEG encoder on a real MI355X: stage 1 against the float64 numpy reference, stage 2 against the plain-Python coder
(byte for byte), whole files through Pillow, hipGraph replay, and the engine's ``encoder="device"`` movie."""
import io
import os
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import _jpeg_ref as J

pytestmark = pytest.mark.gpu

DEV = "cuda"
TIE_BAND = 1.0 / 256          # of a quantisation step: coefficients whose pre-rounding value is this close to a tie are not compared
MAX_EXCLUDED = 0.015          # of a frame's coefficients (a condition on the input, not a tolerance)
# PSNR margin established on the CPU for the reference path against Pillow (tests/test_jpeg_cpu.py: twice the largest gap, 0.1075 dB)
MARGIN_DB = 2 * 0.1075


def ops():
    from latentblending_amd.hip import ops as o
    return o


def frames_for(h, w, seeds=(0,)):
    return [J.make_frame(h, w, sigma, seed=s) for sigma in (0, 6, 40) for s in seeds]


@pytest.mark.parametrize("quality", [75, 92])
@pytest.mark.parametrize("subsampling", ["4:2:0", "4:4:4"])
@pytest.mark.parametrize("h,w", [(512, 512), (1024, 1024), (72, 40), (8, 8)])
def test_stage1_matches_the_float64_reference(h, w, subsampling, quality):
    frames = frames_for(h, w)
    got = ops().jpeg_coefficients_u8(torch.from_numpy(np.stack(frames)).to(DEV), quality, subsampling).cpu().numpy()
    for k, frame in enumerate(frames):
        want, quot = J.reference_coefficients(frame, quality, subsampling)
        assert got[k].shape == want.shape
        frac = np.abs(quot) - np.floor(np.abs(quot))
        near_tie = np.abs(frac - 0.5) <= TIE_BAND
        share = near_tie.mean()
        differ = got[k] != want
        print(f"[jpeg] stage1 {h}x{w} {subsampling} q{quality} frame {k}: near ties {share:.4%}, differing {differ.sum()} "
              f"(outside the band {(differ & ~near_tie).sum()}), max |diff| {np.abs(got[k].astype(int) - want).max()}")
        assert share <= MAX_EXCLUDED
        assert not (differ & ~near_tie).any()
        assert np.abs(got[k].astype(int) - want).max() <= 1


def special_frames(h, w):
    rng = np.random.default_rng(7)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8),            # pure noise: long codes, many stuffed bytes
            np.full((h, w, 3), 137, np.uint8),                           # constant: every block is DC + EOB
            J.make_frame(h, w, 6, seed=2)]


@pytest.mark.parametrize("quality", [92, 100])
@pytest.mark.parametrize("subsampling", ["4:2:0", "4:4:4"])
@pytest.mark.parametrize("h,w", [(8, 8), (72, 40), (40, 72), (128, 256)])
def test_stage2_is_the_reference_coder_byte_for_byte(h, w, subsampling, quality):
    frames = special_frames(h, w)
    coef = ops().jpeg_coefficients_u8(torch.from_numpy(np.stack(frames)).to(DEV), quality, subsampling)
    scans = ops().jpeg_scan_from_coefficients(coef, h, w, subsampling)
    host = coef.cpu().numpy()
    for k in range(len(frames)):
        want = J.entropy_code(host[k], h, w, subsampling)
        assert scans[k] == want, f"frame {k}: {len(scans[k])} bytes against {len(want)}"
    assert any(b"\xff\x00" in s for s in scans)                          # the noise frame did exercise byte stuffing


def test_stage2_survives_coefficients_stage1_cannot_produce():
    """Any int16 input stays inside the worst-case slots (sizes the tables do not hold are coded as garbage, not out of bounds)."""
    h, w = 64, 64
    g = torch.Generator().manual_seed(0)
    n = ops().api.lb_jpeg_coefficient_count(2, h, w, 0) // 2
    coef = torch.randint(-32768, 32768, (2, n // 64, 64), generator=g, dtype=torch.int32).to(torch.int16).to(DEV)
    scans = ops().jpeg_scan_from_coefficients(coef, h, w, "4:2:0")
    assert len(scans) == 2 and all(0 < len(s) <= (n // 64) * 512 + 4 * 16 for s in scans)


@pytest.mark.parametrize("subsampling", ["4:2:0", "4:4:4"])
@pytest.mark.parametrize("h,w", [(512, 512), (72, 40), (8, 8)])
def test_files_decode_like_the_reference_stream(h, w, subsampling):
    frames = frames_for(h, w) + special_frames(h, w)[:2]
    dev = torch.from_numpy(np.stack(frames)).to(DEV)
    files = ops().jpeg_encode_u8(dev, 92, subsampling)
    coef = ops().jpeg_coefficients_u8(dev, 92, subsampling).cpu().numpy()
    assert len(files) == len(frames)
    for k, blob in enumerate(files):
        im = Image.open(io.BytesIO(blob))
        assert im.size == (w, h) and im.mode == "RGB"
        im.load()
        want = J.decode(J.jpeg_file(coef[k], h, w, 92, subsampling))
        assert np.array_equal(np.asarray(im), want)


def test_chunked_encode_equals_one_chunk(monkeypatch):
    o = ops()
    frames = torch.from_numpy(np.stack([J.make_frame(64, 96, 6, seed=s) for s in range(7)])).to(DEV)
    whole = o.jpeg_encode_u8(frames)
    monkeypatch.setattr(o, "_JPEG_WORKSPACE_BUDGET", 3 * o.api.lb_jpeg_workspace_bytes(1, 64, 96, 0))
    assert o.jpeg_encode_u8(frames) == whole


def test_unsupported_size_is_an_error_with_a_message(tmp_path):
    from latentblending_amd import movie
    o = ops()
    frames = torch.zeros((2, 20, 36, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="multiples of 8"):
        o.jpeg_encode_u8(frames)
    with pytest.raises(RuntimeError, match="multiples of 8"):
        o.jpeg_coefficients_u8(frames)
    assert b"multiples of 8" in o.api.lb_last_error_string()
    saver = movie.MovieSaver(str(tmp_path / "odd.avi"), fps=5)
    with pytest.warns(UserWarning, match="encoding on the host"):
        saver.write_frames_device(frames)                                 # Pillow takes over
    saver.finalize()
    assert movie.read_movie_header(str(tmp_path / "odd.avi")) == (5, 20, 36, 2)


def test_graph_replay_equals_eager():
    """Both launchers captured into one graph (no allocation, no synchronisation inside them) replay to the eager bytes."""
    o = ops()
    h, w, n, code = 128, 256, 3, 0
    frames = torch.from_numpy(np.stack([J.make_frame(h, w, 6, seed=s) for s in range(n)])).to(DEV)
    other = torch.from_numpy(np.stack([J.make_frame(h, w, 40, seed=9 + s) for s in range(n)])).to(DEV)
    qt = o._jpeg_qtables(92, frames.device)
    coef = torch.empty(o.api.lb_jpeg_coefficient_count(n, h, w, code), dtype=torch.int16, device=DEV)
    ws = torch.empty(o.api.lb_jpeg_workspace_bytes(n, h, w, code), dtype=torch.uint8, device=DEV)
    out = torch.zeros(n * h * w, dtype=torch.uint8, device=DEV)
    fb = torch.zeros(n, dtype=torch.int32, device=DEV)
    src = frames.clone()

    def run():
        o.jpeg_dct_quant_into(src, qt, coef, code)
        o.jpeg_entropy_into(coef, ws, out, fb, n, h, w, code)

    def result():
        torch.cuda.synchronize()
        sizes = fb.cpu().tolist()
        return sizes, out[:sum(sizes)].cpu().numpy().tobytes()

    run()
    eager_a = result()
    src.copy_(other)
    run()
    eager_b = result()
    assert eager_a != eager_b
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                             # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for want, data in ((eager_a, frames), (eager_b, other)):
        src.copy_(data)
        out.zero_()
        fb.zero_()
        graph.replay()
        assert result() == want
    scans = o.jpeg_scan_from_coefficients(o.jpeg_coefficients_u8(frames), h, w)
    assert b"".join(scans) == eager_a[1] and [len(s) for s in scans] == eager_a[0]


def test_engine_writes_the_movie_on_the_device(tmp_path, monkeypatch):
    """After a native transition ``write_movie_transition(..., encoder="device")`` writes an AVI with duration * fps frames of the
    render size; every decoded frame is as close to the blended source frame as the host path's (Pillow's) frame, within the margin
    the CPU test established; two device-encoded parts concatenate."""
    import sys
    monkeypatch.setenv("LB_TINY_MODEL", "1")
    monkeypatch.chdir(tmp_path)
    for m in [k for k in sys.modules if k == "diffusers" or k.startswith("diffusers.")]:
        del sys.modules[m]
    from diffusers import AutoPipelineForText2Image
    from latentblending_amd import BlendingEngine, movie, utils
    from latentblending_amd.backend import set_backend
    set_backend(None)
    pipe = AutoPipelineForText2Image.from_pretrained("stabilityai/sdxl-turbo", torch_dtype=torch.float16, variant="fp16")
    pipe.to("cuda")
    be = BlendingEngine(pipe, verbose=False)
    be.set_dimensions((128, 128))
    be.set_prompt1("photo of underwater landscape, fish, und the sea, incredible detail, high resolution")
    be.set_prompt2("rendering of an alien planet, strange plants, strange creatures, surreal")
    frames = be.run_transition()
    duration, fps = 2, 15
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.random.seed(11)
        source = utils.add_frames_linear_interp(list(frames), nmb_frames_target=duration * fps)
        np.random.seed(11)
        be.write_movie_transition("host.avi", duration_transition=duration, fps=fps)
        np.random.seed(11)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            be.write_movie_transition("device.avi", duration_transition=duration, fps=fps, encoder="device")
        assert not [w for w in caught if "encoder='device'" in str(w.message)]          # the device path was taken
        be.movie_encoder = "device"
        np.random.seed(12)
        be.write_movie_transition("device2.avi", duration_transition=duration, fps=fps)
        movie.concatenate_movies("both.avi", ["device.avi", "device2.avi"])
    assert movie.read_movie_header("device.avi") == (fps, 128, 128, duration * fps)
    assert movie.read_movie_header("host.avi") == (fps, 128, 128, duration * fps)
    host, dev = movie.read_movie_jpegs("host.avi"), movie.read_movie_jpegs("device.avi")
    assert len(source) == len(host) == len(dev) == duration * fps
    header = movie.jpeg_header(128, 128, 92, "4:2:0")
    for k in range(len(dev)):
        assert dev[k].startswith(header) and not host[k].startswith(header)
        p_dev, p_host = J.psnr(J.decode(dev[k]), source[k]), J.psnr(J.decode(host[k]), source[k])
        if k % 10 == 0:
            print(f"[jpeg] movie frame {k}: device {p_dev:.3f} dB, host {p_host:.3f} dB against the blended source")
        assert p_dev >= p_host - MARGIN_DB
    assert movie.read_movie_header("both.avi") == (fps, 128, 128, 2 * duration * fps)
    both = movie.read_movie_jpegs("both.avi")
    assert both[:len(dev)] == dev and both[len(dev):] == movie.read_movie_jpegs("device2.avi")
    assert os.path.getsize("both.avi") > 10000
