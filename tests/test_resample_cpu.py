"""Host side of the device frame resampler: the numpy restatement of Pillow's 8-bit resampler against Pillow (byte for byte), the
coefficient tables the kernel is fed against the restatement, and the engine's ``size_output`` / ``resample`` arguments on the host
encoder.  No GPU."""
import io
import warnings

import numpy as np
import pytest
from PIL import Image

import _resample_ref as RS
from oracle import pipe as OP
from oracle import sdxl_ref as R

# (Hin, Win) -> (Hout, Wout)
SIZE_PAIRS = [((64, 64), (135, 240)), ((64, 48), (40, 24)), ((24, 40), (24, 100)), ((72, 128), (45, 80)), ((16, 16), (37, 16)),
              ((40, 56), (8, 8)), ((8, 8), (8, 8))]


@pytest.mark.parametrize("name", RS.FILTERS)
@pytest.mark.parametrize("size_in,size_out", SIZE_PAIRS)
def test_restatement_equals_pillow_byte_for_byte(size_in, size_out, name):
    img = RS.random_frames(1, *size_in, seed=size_in[0] + size_out[1])[0]
    got, want = RS.resize(img, size_out, name), RS.pil_resize(img, size_out, name)
    assert got.shape == want.shape == size_out + (3,)
    assert np.array_equal(got, want), f"{int((got != want).sum())} differing bytes"
    if size_in == size_out:
        assert np.array_equal(got, img)                                  # identity: nothing is requantised


@pytest.mark.parametrize("name", RS.FILTERS)
@pytest.mark.parametrize("n_in,n_out", sorted({(a[i], b[i]) for a, b in SIZE_PAIRS for i in (0, 1)} | {(512, 1080), (512, 1920), (1000, 25)}))
def test_tables_agree_with_the_restatement(n_in, n_out, name):
    from latentblending_amd.resample import PRECISION_BITS, resample_tables
    start, count, coef = resample_tables(n_in, n_out, name)
    assert start.dtype == count.dtype == coef.dtype == np.int32
    assert start.shape == count.shape == (n_out,) and coef.shape == (n_out, RS.kmax(n_in, n_out, name))
    want = RS.windows(n_in, n_out, name)
    for i, (lo, ks) in enumerate(want):
        assert (int(start[i]), int(count[i])) == (lo, len(ks)) and coef[i, :len(ks)].tolist() == ks
        assert not coef[i, len(ks):].any()                               # unused tail entries are 0
        assert 0 <= lo and lo + len(ks) <= n_in and 0 < len(ks) <= coef.shape[1]
        assert abs(int(coef[i].sum()) - (1 << PRECISION_BITS)) <= len(ks)      # rounding slack: half a unit per tap at most


def test_bad_arguments_to_the_tables():
    from latentblending_amd.resample import resample_tables
    for args in ((8, 8, "nearest"), (8, 8, None), (0, 8, "box"), (8, -1, "box"), (8, 2.5, "box")):
        with pytest.raises(ValueError):
            resample_tables(*args)


@pytest.fixture(scope="module")
def engine():
    """An engine on the CPU oracle pipe whose key frames are seven host numpy frames of 64 x 40 (no transition is run)."""
    from latentblending_amd import BlendingEngine
    from latentblending_amd.backend import set_backend
    set_backend(R.TorchCpuBackend())
    try:
        pipe = OP.StableDiffusionXLPipeline(turbo=True, unet_cfg=R.tiny_unet_cfg(), vae_cfg=R.tiny_vae_cfg())
        be = BlendingEngine(pipe, metric=R.OracleLPIPS(7), verbose=False)
        be.set_dimensions((64, 40))
        be.tree_final_imgs = list(RS.random_frames(7, 40, 64, seed=4) // 2 + np.arange(7, dtype=np.uint8)[:, None, None, None] * 10)
        yield be
    finally:
        set_backend(None)


def test_engine_defaults_and_session_fields(engine):
    from latentblending_amd.session import _ENGINE_FIELDS
    assert engine.movie_size is None and engine.movie_resample == "bicubic"
    assert {"movie_encoder", "movie_size", "movie_resample"} <= set(_ENGINE_FIELDS)


@pytest.mark.parametrize("name", ["bicubic", "lanczos"])
def test_host_movie_at_another_size(engine, tmp_path, name):
    """48 x 32 from 64 x 40 key frames: header, frame count, and every KEY frame of the movie is the JPEG of Pillow's resize of
    that key frame (the key frames are resized, then in-betweened at the output size)."""
    from latentblending_amd import movie, utils
    fp = str(tmp_path / "small.avi")
    np.random.seed(2)
    engine.write_movie_transition(fp, duration_transition=2, fps=10, encoder="host", size_output=(48, 32), resample=name)
    assert movie.read_movie_header(fp) == (10, 32, 48, 20)
    jpegs = movie.read_movie_jpegs(fp)
    assert len(jpegs) == 20
    for blob in (jpegs[0], jpegs[-1]):
        im = Image.open(io.BytesIO(blob))
        im.load()
        assert im.size == (48, 32) and im.mode == "RGB"
    keys = [RS.pil_resize(k, (32, 48), name) for k in engine.tree_final_imgs]
    np.random.seed(2)
    want = utils.add_frames_linear_interp(keys, nmb_frames_target=20)
    saver = movie.AviMovieSaver(str(tmp_path / "want.avi"), fps=10, shape_hw=[32, 48])
    for frame in want:
        saver.write_frame(frame)
    assert saver._jpegs == jpegs
    assert np.array_equal(want[0], keys[0]) and np.array_equal(want[-1], keys[-1])


def test_attributes_are_the_defaults_of_the_arguments(engine, tmp_path):
    from latentblending_amd import movie
    blobs = []
    try:
        for k, kw in enumerate(({"size_output": (24, 16), "resample": "box"}, {})):
            np.random.seed(3)
            engine.write_movie_transition(str(tmp_path / f"{k}.avi"), duration_transition=1, fps=12, **kw)
            blobs.append(open(tmp_path / f"{k}.avi", "rb").read())
            engine.movie_size, engine.movie_resample = (24, 16), "box"
    finally:
        engine.movie_size, engine.movie_resample = None, "bicubic"
    assert blobs[0] == blobs[1] and movie.read_movie_header(str(tmp_path / "1.avi")) == (12, 16, 24, 12)


def test_no_size_writes_the_file_of_the_unchanged_path(engine, tmp_path):
    """``size_output=None, resample=None`` is the call without them, byte for byte, from the same seeded RNG."""
    blobs = []
    for k, kw in enumerate(({}, {"size_output": None, "resample": None}, {"encoder": "host", "size_output": None})):
        np.random.seed(5)
        engine.write_movie_transition(str(tmp_path / f"{k}.avi"), duration_transition=1, fps=15, **kw)
        blobs.append(open(tmp_path / f"{k}.avi", "rb").read())
    assert blobs[0] == blobs[1] == blobs[2]
    # ... and it is the file the plain in-between + writer sequence gives (what the method did before it took a size)
    from latentblending_amd import movie
    np.random.seed(5)
    frames = movie.fill_up_frames_linear_interpolation(engine.tree_final_imgs, 1, 15)
    saver = movie.MovieSaver(str(tmp_path / "plain.avi"), fps=15, shape_hw=[40, 64])
    for frame in frames:
        saver.write_frame(frame)
    saver.finalize()
    assert open(tmp_path / "plain.avi", "rb").read() == blobs[0]


def test_device_encoder_without_device_frames_falls_back_at_the_output_size(engine, tmp_path):
    from latentblending_amd import movie
    out = {}
    for enc in ("host", "device"):
        np.random.seed(6)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            engine.write_movie_transition(str(tmp_path / f"{enc}.avi"), duration_transition=1, fps=10, encoder=enc, size_output=(48, 32))
        assert len([w for w in caught if "encoder='device'" in str(w.message)]) == (1 if enc == "device" else 0)
        out[enc] = open(tmp_path / f"{enc}.avi", "rb").read()
    assert out["host"] == out["device"] and movie.read_movie_header(str(tmp_path / "device.avi")) == (10, 32, 48, 10)


@pytest.mark.parametrize("kw", [{"resample": "nearest"}, {"resample": 3}, {"size_output": (0, 32)}, {"size_output": (48, -8)},
                                {"size_output": (48,)}, {"size_output": (48.5, 32)}, {"size_output": 48}])
@pytest.mark.parametrize("encoder", ["host", "device"])
def test_bad_filter_or_size_raises_before_anything_happens(engine, tmp_path, kw, encoder):
    np.random.seed(9)
    state = np.random.get_state()
    with pytest.raises(ValueError):
        engine.write_movie_transition(str(tmp_path / "bad.avi"), duration_transition=1, fps=10, encoder=encoder, **kw)
    with pytest.raises(ValueError):
        engine.write_imgs_transition(str(tmp_path / "bad_imgs"), **kw)
    assert not (tmp_path / "bad.avi").exists() and not (tmp_path / "bad_imgs").exists()
    after = np.random.get_state()
    assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]


def test_write_imgs_at_another_size(engine, tmp_path):
    engine.write_imgs_transition(str(tmp_path / "imgs"), size_output=(40, 24), resample="bilinear")
    files = sorted((tmp_path / "imgs").iterdir())
    assert [f.name for f in files] == [f"lowres_img_{k:04d}.jpg" for k in range(7)]
    for f, key in zip(files, engine.tree_final_imgs):
        im = Image.open(f)
        assert im.size == (40, 24)
        buf = io.BytesIO()
        Image.fromarray(RS.pil_resize(key, (24, 40), "bilinear")).save(buf, format="JPEG")
        assert f.read_bytes() == buf.getvalue()
    engine.write_imgs_transition(str(tmp_path / "plain"))                # unchanged without a size
    assert Image.open(tmp_path / "plain" / "lowres_img_0000.jpg").size == (64, 40)


def test_replay_and_frontend_take_the_size():
    import inspect
    from latentblending_amd import frontend, replay
    for fn in (replay.run_multi_transition, replay.run_movie_json, frontend.BlendingVariableHolder.generate_movie):
        params = inspect.signature(fn).parameters
        assert params["movie_size"].default is None and params["movie_resample"].default is None
