"""Host side of the device MJPEG encoder: tables, header, the reference coder's quality against Pillow, the container and
the engine's ``encoder`` switch.  No GPU."""
import io
import warnings

import numpy as np
import pytest
from PIL import Image, JpegImagePlugin

import _jpeg_ref as J
from oracle import pipe as OP
from oracle import sdxl_ref as R

# Largest |PSNR(Pillow) - PSNR(reference coder)| measured on PSNR_CASES (float64 DCT against libjpeg's integer DCT): 0.1075 dB, on the
# noise-free frame (where the reference is the better one); 0.040 dB at most on the noisy frames.  The bar is twice that.
LARGEST_GAP_DB = 0.1075
MARGIN_DB = 2 * LARGEST_GAP_DB

PSNR_CASES = [(512, 512, 6), (512, 512, 40), (72, 40, 6), (128, 128, 0)]


@pytest.mark.parametrize("quality", [50, 75, 92, 100])
def test_tables_equal_pillow(quality):
    from latentblending_amd.movie import jpeg_tables
    buf = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, format="JPEG", quality=quality)
    q = Image.open(io.BytesIO(buf.getvalue())).quantization
    luma, chroma = jpeg_tables(quality)
    assert list(q[0]) == list(luma) and list(q[1]) == list(chroma)


@pytest.mark.parametrize("subsampling,code", [("4:2:0", 2), ("4:4:4", 0)])
@pytest.mark.parametrize("h,w", [(64, 64), (40, 72), (72, 40), (8, 8)])
def test_header_and_reference_scan_open_in_pillow(h, w, subsampling, code):
    from latentblending_amd.movie import jpeg_header
    frame = J.make_frame(h, w, 6, seed=3)
    coef, _ = J.reference_coefficients(frame, 92, subsampling)
    blob = jpeg_header(h, w, 92, subsampling) + J.entropy_code(coef, h, w, subsampling) + b"\xff\xd9"
    im = Image.open(io.BytesIO(blob))
    assert im.size == (w, h) and im.mode == "RGB" and JpegImagePlugin.get_sampling(im) == code
    im.load()
    assert J.psnr(np.asarray(im), frame) > 28.0          # the right picture, not just a decodable one


@pytest.mark.parametrize("subsampling", ["4:2:0", "4:4:4"])
@pytest.mark.parametrize("h,w,sigma", PSNR_CASES)
def test_reference_design_is_as_good_as_pillow(h, w, sigma, subsampling):
    """The design (float DCT, round half away from zero, plain 2x2 chroma mean, standard tables) against Pillow's own encode at the
    same quality and sampling with restart_marker_rows=1.  Measured (PSNR against the source, dB; reference coder / Pillow):
      512x512 sigma 6   4:2:0 32.917 / 32.887   4:4:4 33.779 / 33.739
      512x512 sigma 40  4:2:0 18.264 / 18.262   4:4:4 31.834 / 31.812
      72x40   sigma 6   4:2:0 32.894 / 32.889   4:4:4 33.764 / 33.740
      128x128 sigma 0   4:2:0 48.782 / 48.674   4:4:4 49.840 / 49.858
    largest gap 0.1075 dB; bar = Pillow - 2 * 0.1075 dB."""
    frame = J.make_frame(h, w, sigma, seed=1)
    coef, _ = J.reference_coefficients(frame, 92, subsampling)
    ours = J.psnr(J.decode(J.jpeg_file(coef, h, w, 92, subsampling)), frame)
    pillow = J.psnr(J.decode(J.pillow_encode(frame, 92, subsampling)), frame)
    print(f"[jpeg] {h}x{w} sigma {sigma} {subsampling}: reference coder {ours:.3f} dB, Pillow {pillow:.3f} dB, gap {pillow - ours:+.4f}")
    assert ours >= pillow - MARGIN_DB


def test_write_jpeg_round_trips_through_the_container(tmp_path):
    from latentblending_amd import movie
    frames = [J.make_frame(40, 72, 6, seed=s) for s in range(5)]
    jpegs = [J.jpeg_file(J.reference_coefficients(f)[0], 40, 72) for f in frames]
    paths = []
    for part in range(2):
        fp = str(tmp_path / f"part{part}.avi")
        saver = movie.MovieSaver(fp, fps=12, shape_hw=[40, 72])
        for j in jpegs[part * 2:part * 2 + 3]:
            saver.write_jpeg(j)
        saver.finalize()
        paths.append(fp)
        assert movie.read_movie_header(fp) == (12, 40, 72, 3)
        assert movie.read_movie_jpegs(fp) == jpegs[part * 2:part * 2 + 3]
    fp_all = str(tmp_path / "all.avi")
    movie.concatenate_movies(fp_all, paths)
    assert movie.read_movie_header(fp_all) == (12, 40, 72, 6)
    assert movie.read_movie_jpegs(fp_all) == jpegs[0:3] + jpegs[2:5]
    for j in movie.read_movie_jpegs(fp_all):
        assert J.decode(j).shape == (40, 72, 3)
    with pytest.raises(ValueError):
        movie.MovieSaver(str(tmp_path / "x.avi"), fps=12, shape_hw=[40, 72]).write_jpeg(b"not a jpeg")


def test_container_bytes_match_the_chunk_by_chunk_layout(tmp_path):
    """finalize() joins its pieces once; the file is the RIFF layout written out chunk by chunk (odd payloads padded)."""
    import struct
    from latentblending_amd import movie
    jpegs = [b"\xff\xd8" + bytes([i]) * (5 + i) + b"\xff\xd9" for i in range(4)]       # odd and even lengths
    fp = str(tmp_path / "m.avi")
    saver = movie.MovieSaver(fp, fps=30, shape_hw=[8, 8])
    for j in jpegs:
        saver.write_jpeg(j)
    saver.finalize()
    data = open(fp, "rb").read()
    assert data[:4] == b"RIFF" and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    assert movie.read_movie_jpegs(fp) == jpegs
    i = data.index(b"idx1")
    assert struct.unpack("<I", data[i + 4:i + 8])[0] == 16 * len(jpegs) and i + 8 + 16 * len(jpegs) == len(data)
    movi = data.index(b"movi")
    for k, j in enumerate(jpegs):
        _, _, off, size = struct.unpack("<4sIII", data[i + 8 + 16 * k:i + 24 + 16 * k])
        assert size == len(j) and data[movi + off:movi + off + 4] == b"00dc" and data[movi + off + 8:movi + off + 8 + size] == j


def test_engine_encoder_switch_on_a_cpu_pipe(tmp_path):
    """``encoder="host"`` and the unset default write the same bytes; "device" without device-resident frames warns once and
    writes the host file."""
    from latentblending_amd import BlendingEngine
    from latentblending_amd.backend import set_backend
    from latentblending_amd.session import _ENGINE_FIELDS
    set_backend(R.TorchCpuBackend())
    try:
        pipe = OP.StableDiffusionXLPipeline(turbo=True, unet_cfg=R.tiny_unet_cfg(), vae_cfg=R.tiny_vae_cfg())
        np.random.seed(0)
        be = BlendingEngine(pipe, metric=R.OracleLPIPS(7), verbose=False)
        assert be.movie_encoder == "host" and "movie_encoder" in _ENGINE_FIELDS
        be.set_dimensions((64, 64))
        be.set_branching(nmb_max_branches=3)
        be.set_prompt1("a reef")
        be.set_prompt2("an alien planet")
        be.run_transition(fixed_seeds=[1, 2])
        blobs = {}
        for name, kw in (("default", {}), ("host", {"encoder": "host"}), ("device", {"encoder": "device"})):
            fp = str(tmp_path / f"{name}.avi")
            np.random.seed(5)
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                be.write_movie_transition(fp, duration_transition=1, fps=10, **kw)
            fallbacks = [w for w in caught if "encoder='device'" in str(w.message)]
            assert len(fallbacks) == (1 if name == "device" else 0)
            blobs[name] = open(fp, "rb").read()
        assert blobs["default"] == blobs["host"] == blobs["device"]
        be.movie_encoder = "device"                       # the attribute is what encoder=None reads
        with pytest.warns(UserWarning, match="encoder='device'"):
            np.random.seed(5)
            be.write_movie_transition(str(tmp_path / "attr.avi"), duration_transition=1, fps=10)
        assert open(tmp_path / "attr.avi", "rb").read() == blobs["host"]
        with pytest.raises(ValueError):
            be.write_movie_transition(str(tmp_path / "bad.avi"), duration_transition=1, encoder="gpu")
    finally:
        set_backend(None)


def test_inbetween_plan_is_shared_and_draws_once(monkeypatch):
    """``add_frames_linear_interp`` returns what it returned before the plan was factored out (same frames from the same seeded
    RNG, one ``np.random.rand`` call per attempt), and ``inbetween_frames_device`` declines host frames before touching the RNG."""
    from latentblending_amd import utils
    imgs = [J.make_frame(16, 16, 6, seed=s) for s in range(4)]
    np.random.seed(3)
    out = utils.add_frames_linear_interp(list(imgs), nmb_frames_target=11)
    assert len(out) == 11 and all(o.dtype == np.uint8 for o in out)
    np.random.seed(3)
    draw = np.random.rand(3)
    per_gap = (np.where(draw > 1 - (7 / 3 - 2), 1.0, 0.0) + 2).astype(int)
    assert per_gap.sum() == 7                              # (seed 3 hits the total at the first draw)
    k = 0
    for g in range(3):
        for wgt in np.linspace(0, 1, per_gap[g] + 2)[:-1]:
            want = ((1 - wgt) * imgs[g].astype(np.float32) + wgt * imgs[g + 1].astype(np.float32)).astype(np.uint8) if wgt else imgs[g]
            assert np.array_equal(out[k], want)
            k += 1
    assert np.array_equal(out[-1], imgs[-1])
    state = np.random.get_state()[1].copy()
    assert utils.inbetween_frames_device(imgs, 11) is None
    assert np.array_equal(np.random.get_state()[1], state)
