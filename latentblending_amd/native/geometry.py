"""Latent geometry of the native launch programs: (H, W) sizes, their validity, and the rule that sends a 3x3 conv of a
non-square program to the ragged-tile form of the halo kernel.  Pure host arithmetic (no torch, no library)."""
from __future__ import annotations

from typing import Tuple, Union

Size = Union[int, Tuple[int, int]]

# Smallest tile fill (valid pixels / tile pixels of the ragged launch) at which an emitter prefers the ragged halo kernel to the
# implicit GEMM.  From profiles/nonsquare.txt (tools/nonsquare_bench.py on one MI355X: the resnet conv of every ragged UNet level
# of the 1344x768, 1024x576 and 768x448 renders; implicit GEMM time / ragged halo time):
#   level HxW    C     B  tile   blocks  fill   speedup
#   96 x 168    320    2  16x16   396   0.955    1.15
#   48 x 84     640    2  32x8    180   0.875    1.60
#   24 x 42    1280    2  32x8    120   0.656    1.14
#   36 x 64     640    2  32x8    100   0.900    1.12
#   18 x 32    1280    2  32x8     60   0.750    0.61   <- 60 blocks: lb_gemm_f16 keeps it on the implicit GEMM (LB_HALO_MIN_BLOCKS = 96)
#   28 x 48     640   17  16x16   510   0.875    1.41
#   14 x 24    1280   17  32x8    340   0.656    1.25
# No crossover in the fill: the lowest fills measured (0.656) win, and the one loss is a grid of 60 blocks on 256 CUs, which the
# router's chip-filling threshold already sends to the implicit GEMM whatever the emitter asks for.  So the constant is 0.
HALO_RAGGED_MIN_FILL = 0.0


TILEABLE_WRAP = {"": 0, "x": 1, "y": 2, "xy": 3}     # the ``tileable`` setting -> ``ConvGeom.wrap`` bits (bit 0: columns, bit 1: rows)


def check_tileable(value, who: str = "NativeSDXLPipe") -> str:
    """The ``tileable`` setting as the pipe keeps it: None / False / "" -> "" (off); "x", "y", "xy" (case-insensitive) ->
    themselves; True -> "xy".  Anything else raises a ``ValueError`` that names the valid values."""
    if value is None or value is False:
        return ""
    if value is True:
        return "xy"
    if isinstance(value, str) and value.strip().lower() in TILEABLE_WRAP:
        return value.strip().lower()
    raise ValueError(f"{who}: tileable must be None / False / '' (off), 'x', 'y', 'xy' or True (= 'xy'), got {value!r}")


def latent_hw(size: Size) -> Tuple[int, int]:
    """A side ``L`` (meaning L x L) or a pair ``(H, W)`` in latent pixels -> ``(H, W)``."""
    if isinstance(size, (tuple, list)):
        if len(size) != 2:
            raise ValueError(f"latent size must be a side L or a pair (H, W), got {size!r}")
        h, w = int(size[0]), int(size[1])
    else:
        h = w = int(size)
    if h <= 0 or w <= 0:
        raise ValueError(f"latent size must be positive, got {size!r}")
    return h, w


def program_key(B: int, size: Size) -> Tuple[int, ...]:
    """Cache key of a launch program: ``(B, H, W)`` - ``L`` and ``(L, L)`` name the same program.  A SQUARE program keeps the
    two-element key ``(B, L)`` it always had: bench.py and tools/ unpack the caches' keys as ``(B, L)`` and hand them back to
    ``unet_program(B, L)`` / ``vae_program(B, L)``."""
    h, w = latent_hw(size)
    return (int(B), h) if h == w else (int(B), h, w)


def check_unet_latent_size(H: int, W: int, levels: int, pixels_per_latent: int = 8) -> None:
    """Each of the UNet's ``levels - 1`` downsamplers halves the map and each upsampler doubles it: a side that is not a multiple
    of ``2 ** (levels - 1)`` comes back from the up path with another size than its skip connection.  Raises ``ValueError``
    naming the two nearest valid sizes."""
    m = 2 ** (max(int(levels), 1) - 1)
    if H % m == 0 and W % m == 0:
        return

    def near(v):
        lo, hi = max(v // m * m, m), (v + m - 1) // m * m
        return lo, hi
    (hl, hh), (wl, wh) = near(H), near(W)
    k = int(pixels_per_latent)
    raise ValueError(
        f"native UNet: latent size {H} x {W} (H x W) is not valid: both sides must be multiples of {m} "
        f"(render sizes multiples of {m * k}); nearest valid latent sizes: {hl} x {wl} and {hh} x {wh} "
        f"(renders {wl * k}x{hl * k} and {wh * k}x{hh * k}, width x height)")


def halo_tile_shape(H: int, W: int) -> Tuple[int, int]:
    """(tile height, tile width) the 3x3 halo kernel uses for an H x W image under LB_GEMM_HALO_RAGGED - the host twin of
    lb_conv3x3_halo_eligible: a shape that divides keeps its tile, otherwise the shape with fewer tiles, ties to 32 wide."""
    if W % 32 == 0 and H % 8 == 0:
        return 8, 32
    if W % 16 == 0 and H % 16 == 0:
        return 16, 16
    t32 = -(-W // 32) * -(-H // 8)
    t16 = -(-W // 16) * -(-H // 16)
    return (16, 16) if t16 < t32 else (8, 32)


def halo_ragged_fill(H: int, W: int, tile_w: int) -> float:
    """Valid pixels / tile pixels of an H x W image covered by 256-pixel tiles ``tile_w`` wide (1.0 = it divides)."""
    th = 256 // tile_w
    return (H * W) / float(-(-H // th) * -(-W // tile_w) * 256)


def use_ragged_halo(nonsquare: bool, kind_plain: int, kind_ragged: int, H: int, W: int, tile_w: int,
                    min_fill: float = HALO_RAGGED_MIN_FILL) -> bool:
    """The emitters' rule for one 3x3 / stride 1 conv: set LB_GEMM_HALO_RAGGED only in a non-square program, only where the
    halo kernel refuses the shape without the flag (``kind_plain`` 0) and takes it with the flag (``kind_ragged`` 3), and only
    at a tile fill of at least ``min_fill``.  ``kind_*`` / ``tile_w`` as reported by lb_conv_halo_plan."""
    if not nonsquare or kind_plain != 0 or kind_ragged != 3 or tile_w not in (16, 32):
        return False
    return halo_ragged_fill(H, W, tile_w) >= min_fill
