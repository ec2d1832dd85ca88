"""Device frame resampler on a real MI355X: ``ops.resample_u8`` against ``PIL.Image.resize`` (identical bytes, no tolerance), its
memory contract inside guard bands, and the movie / image writers at another output size."""
import io
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import _guard as G
import _resample_ref as RS

pytestmark = pytest.mark.gpu

DEV = "cuda"


def ops():
    from latentblending_amd.hip import ops as o
    return o


_WANT = {}


def pillow(frames, size_hw, name):
    """Pillow's resize of every frame (computed once per case, shared, never written to)."""
    key = (frames.shape, frames[:, :2, :2].tobytes(), size_hw, name)
    if key not in _WANT:
        _WANT[key] = np.stack([RS.pil_resize(f, size_hw, name) for f in frames])
        _WANT[key].setflags(write=False)
    return _WANT[key]


def check(frames, size_hw, name):
    got = ops().resample_u8(torch.from_numpy(frames).to(DEV), size_hw, name)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (frames.shape[0],) + tuple(size_hw) + (3,)
    got, want = got.cpu().numpy(), pillow(frames, size_hw, name)
    differ = got != want
    print(f"[resample] {frames.shape[1:3]} -> {size_hw} {name} n={frames.shape[0]}: {int(differ.sum())} differing bytes of {want.size}")
    assert not differ.any(), f"first differing byte at (frame, y, x, c) = {tuple(np.argwhere(differ)[0])}"
    return got


@pytest.mark.parametrize("name", RS.FILTERS)
@pytest.mark.parametrize("size_in,size_out", [((24, 40), (37, 100)), ((72, 128), (45, 80)), ((64, 48), (40, 24)), ((17, 23), (31, 9))])
def test_equals_pillow(size_in, size_out, name):
    """Odd sizes, rows that are no multiple of 4 bytes (37 * 3, 9 * 3) and rows that are (100 * 3, 80 * 3, 24 * 3: the dword
    form of the vertical pass), up- and downscaling in one call, windows cut off at the edges."""
    check(RS.random_frames(3, *size_in, seed=1), size_out, name)


@pytest.mark.parametrize("name", RS.FILTERS)
@pytest.mark.parametrize("size_in,size_out", [((24, 40), (24, 100)), ((24, 40), (50, 40)), ((16, 16), (16, 16))])
def test_a_pass_whose_axis_keeps_its_size_is_skipped(size_in, size_out, name):
    frames = RS.random_frames(3, *size_in, seed=2)
    got = check(frames, size_out, name)
    if size_in == size_out:
        assert np.array_equal(got, frames)


@pytest.mark.parametrize("name", ["bicubic", "lanczos"])
def test_overshoot_clips(name):
    """8-pixel black / white checkerboard, 32 x 32 -> 75 x 75: the negative lobes overshoot below 0 and above 255."""
    yy, xx = np.mgrid[0:32, 0:32]
    board = np.where(((yy // 8) + (xx // 8)) % 2 == 0, 0, 255).astype(np.uint8)
    frames = np.ascontiguousarray(np.broadcast_to(board[None, :, :, None], (2, 32, 32, 3)))
    got = check(frames, (75, 75), name)
    assert got.min() == 0 and got.max() == 255 and len(np.unique(got)) > 2


def test_long_windows():
    """7 x downscale with Lanczos: 21 and more taps per output sample, both ways."""
    o = ops()
    check(RS.random_frames(3, 40, 56, seed=3), (8, 8), "lanczos")
    assert o._resample_tables(40, 56, 8, 8, "lanczos", torch.device(DEV))[0][1].max().item() >= 21


def test_windows_too_long_for_a_full_band():
    """2400 -> 60 columns with Lanczos: 241 coefficients per output pixel, so a block stages 50 pixels' rows, not 64."""
    check(RS.random_frames(2, 3, 2400, seed=5), (5, 60), "lanczos")


@pytest.mark.parametrize("n", [1, 17])
def test_every_frame_of_a_stack(n):
    check(RS.random_frames(n, 64, 64, seed=n), (96, 128), "bicubic")


@pytest.mark.parametrize("name", ["bilinear", "lanczos"])
@pytest.mark.parametrize("size_in,size_out", [((17, 23), (31, 9)), ((24, 40), (37, 100))])
def test_memory_contract(size_in, size_out, name):
    """dst and tmp inside guard bands, src followed by a poisoned tail: the guards stay intact, the result is Pillow's whatever
    the guards and the tail hold (two sentinels: 0xA5 and 0x3C are both legal pixel values)."""
    o = ops()
    n = 3
    (hin, win), (hout, wout) = size_in, size_out
    frames = RS.random_frames(n, hin, win, seed=6)
    want = pillow(frames, size_out, name)
    tx, ty = o._resample_tables(hin, win, hout, wout, name, torch.device(DEV))
    flat = torch.from_numpy(frames).reshape(1, -1)
    for sentinel in (0xA5, 0x3C):
        src = G.poisoned(flat, 1, flat.shape[1], flat.shape[1], sentinel, device=DEV, extra_rows=1).view(n, hin, win, 3)
        tmp, tmp_guard = G.guarded(1, n * hin * wout * 3, n * hin * wout * 3, torch.uint8, DEV, back_rows=1, sentinel=sentinel)
        dst, dst_guard = G.guarded(1, n * hout * wout * 3, n * hout * wout * 3, torch.uint8, DEV, back_rows=1, sentinel=sentinel)
        assert src.is_contiguous() and tmp.is_contiguous() and dst.is_contiguous()
        o.resample_u8_into(src, tmp.view(n, hin, wout, 3), dst.view(n, hout, wout, 3), tx, ty)
        torch.cuda.synchronize()
        tmp_guard.assert_intact("tmp")
        dst_guard.assert_intact("dst")
        assert np.array_equal(dst.view(n, hout, wout, 3).cpu().numpy(), want)
        assert np.array_equal(tmp.view(n, hin, wout, 3).cpu().numpy(), pillow(frames, (hin, wout), name))


def test_refusals_leave_the_result_alone():
    o = ops()
    frames = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=DEV)
    tx, ty = o._resample_tables(8, 8, 12, 12, "box", frames.device)
    dst, guard = G.guarded(1, 2 * 12 * 12 * 3, 2 * 12 * 12 * 3, torch.uint8, DEV, back_rows=1)
    with pytest.raises(RuntimeError, match="tmp"):
        o.resample_u8_into(frames, None, dst.view(2, 12, 12, 3), tx, ty)
    with pytest.raises(RuntimeError, match="horizontal tables"):
        o.resample_u8_into(frames, frames, dst.view(2, 12, 12, 3), None, ty)
    with pytest.raises(RuntimeError, match="vertical tables"):
        o.resample_u8_into(frames, frames, dst.view(2, 12, 12, 3), tx, None)
    torch.cuda.synchronize()
    guard.assert_untouched("dst")
    for bad in ((0, 8), (8, -1)):
        with pytest.raises(ValueError):
            o.resample_u8(frames, bad)
    with pytest.raises(ValueError):
        o.resample_u8(frames, (8, 8), "nearest")


def device_keys(frames):
    from latentblending_amd.native.frames import DeviceImage
    return [DeviceImage(torch.from_numpy(f).to(DEV)) for f in frames]


class EngineStandIn:
    """What the writers read of an engine, around the engine's own methods (no model is loaded)."""
    verbose = False
    movie_encoder = "host"
    movie_size = None
    movie_resample = "bicubic"

    def __init__(self, frames, h, w):
        import types
        from latentblending_amd.blending_engine import BlendingEngine
        for name in ("write_movie_transition", "_write_movie_transition_device", "write_imgs_transition", "_movie_output"):
            setattr(self, name, types.MethodType(getattr(BlendingEngine, name), self))
        self.tree_final_imgs = frames
        self.dh = types.SimpleNamespace(height_img=h, width_img=w)


def test_resize_frames_device_declines_host_frames():
    from latentblending_amd import utils
    frames = RS.random_frames(3, 16, 16, seed=7)
    assert utils.resize_frames_device(list(frames), (8, 8), "box") is None
    assert utils.resize_frames_device(torch.from_numpy(frames), (8, 8), "box") is None
    keys = device_keys(frames)
    for source in (keys, torch.from_numpy(frames).to(DEV)):
        got = utils.resize_frames_device(source, (8, 24), "box")
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), pillow(frames, (8, 24), "box"))


def test_device_movie_at_another_size(tmp_path):
    """17 device key frames of 48 x 48 -> a 96 x 64 movie of 60 frames through resize_frames_device, inbetween_frames_device and the
    device encoder: the JPEGs in the file are the device encoder's output for the Pillow-resized, then blended frames."""
    from latentblending_amd import movie, utils
    o = ops()
    frames = RS.random_frames(17, 48, 48, seed=8) // 4 + np.linspace(0, 190, 17).astype(np.uint8)[:, None, None, None]
    eng = EngineStandIn(device_keys(frames), 48, 48)
    fp = str(tmp_path / "wide.avi")
    np.random.seed(4)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        eng.write_movie_transition(fp, duration_transition=2, fps=30, encoder="device", size_output=(96, 64))
    assert not [w for w in caught if "encoder='device'" in str(w.message) or "on the host" in str(w.message)]
    assert movie.read_movie_header(fp) == (30, 64, 96, 60)
    keys = torch.from_numpy(pillow(frames, (64, 96), "bicubic").copy()).to(DEV)
    np.random.seed(4)
    per_gap = utils._insert_plan(16, 60)
    left, weights = utils._lerp_plan(per_gap)
    blended = torch.cat([o.frames_lerp_u8(keys, left, weights), keys[-1:]])
    assert movie.read_movie_jpegs(fp) == o.jpeg_encode_u8(blended)
    # the steps one by one give the same stack
    np.random.seed(4)
    stack = utils.inbetween_frames_device(utils.resize_frames_device(eng.tree_final_imgs, (64, 96), "bicubic"), 60)
    assert torch.equal(stack, blended)
    # the attributes are the arguments' defaults, and the host encoder writes the same frames at that size
    eng.movie_encoder, eng.movie_size = "device", (96, 64)
    np.random.seed(4)
    eng.write_movie_transition(str(tmp_path / "attr.avi"), duration_transition=2, fps=30)
    assert open(tmp_path / "attr.avi", "rb").read() == open(fp, "rb").read()


def test_device_movie_at_a_size_the_encoder_does_not_take(tmp_path):
    """100 x 60 (60 is no multiple of 8): resized and blended on the device, encoded by the writer's own host fall-back."""
    from latentblending_amd import movie
    frames = RS.random_frames(5, 48, 48, seed=9)
    eng = EngineStandIn(device_keys(frames), 48, 48)
    np.random.seed(1)
    with pytest.warns(UserWarning, match="encoding on the host"):
        eng.write_movie_transition(str(tmp_path / "odd.avi"), duration_transition=1, fps=12, encoder="device", size_output=(100, 60))
    assert movie.read_movie_header(str(tmp_path / "odd.avi")) == (12, 60, 100, 12)
    first = Image.open(io.BytesIO(movie.read_movie_jpegs(str(tmp_path / "odd.avi"))[0]))
    buf = io.BytesIO()
    Image.fromarray(pillow(frames, (60, 100), "bicubic")[0]).save(buf, format="JPEG", quality=92)
    assert first.size == (100, 60) and movie.read_movie_jpegs(str(tmp_path / "odd.avi"))[0] == buf.getvalue()


def test_write_imgs_at_another_size(tmp_path):
    frames = RS.random_frames(4, 48, 48, seed=10)
    eng = EngineStandIn(device_keys(frames), 48, 48)
    eng.write_imgs_transition(str(tmp_path / "imgs"), size_output=(40, 24))
    files = sorted((tmp_path / "imgs").iterdir())
    assert len(files) == 4
    want = pillow(frames, (24, 40), "bicubic")
    for k, f in enumerate(files):
        assert Image.open(f).size == (40, 24)
        buf = io.BytesIO()
        Image.fromarray(want[k]).save(buf, format="JPEG")
        assert f.read_bytes() == buf.getvalue()
