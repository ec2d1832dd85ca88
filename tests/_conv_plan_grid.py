"""The grid of tests/test_conv_plan_cpu.py: shapes, flags and switch settings - no library call, no expectation.

A row is (kind, B, H, W, cin, cout, options): ``kind`` names the conv form (KINDS below), H x W is the INPUT map, ``options`` a
dict of the few things besides the geometry that a plan reads: ``flags`` (base flags of the row), ``residual`` / ``rowvec``
(pointers whose nullness counts), ``partial`` (True / False; default: the emitter's rule - a split-K workspace for grids of at
most 640 64 x 64 tiles) and ``zero_page`` (default True)."""

# kind -> (KH = KW, stride, pad, ups, scatter); "gemm" / "geglu": no conv (M = B, N = cout, K = cin; H = W = 0)
KINDS = {
    "c3": (3, 1, 1, 0, 0),          # 3x3 / stride 1 / pad 1
    "c3s2": (3, 2, 1, 0, 0),        # downsampler
    "c3ups": (3, 1, 1, 1, 0),       # nearest-2x upsample fused into the gather (tiny decoder)
    "up2all": (2, 1, 0, 0, 2),      # sub-pixel upsampler, all four parities in one launch
    "up2par": (2, 1, 0, 0, 1),      # one parity of the sub-pixel upsampler (implicit GEMM)
}

# flag bits as in include/lb_hip.h (tests/test_conv_plan_cpu.py checks them against hip/lib.py)
OUT_F32, RES_F32, GEGLU, RELU, RAGGED, C64, KSPLIT, GN_A = 1, 2, 4, 32, 1024, 2048, 4096, 8192
FLAG_SETS = [0, RAGGED, KSPLIT, RAGGED | KSPLIT, GN_A]

# switch settings, each one step away from the defaults: (lb_gemm_set_halo, lb_conv_halo_set_ksplit (mode, grid),
# lb_conv_halo_set_gn_a (mode, grid), lb_gemm_set_tuning (tile, splitk))
DEFAULTS = {"halo": 1, "ksplit": (1, 0), "gn_a": (1, 0), "tuning": (0, 0)}
SETTINGS = [
    ("default", {}),
    ("halo_0", {"halo": 0}), ("halo_2", {"halo": 2}),
    ("ksplit_0", {"ksplit": (0, 0)}), ("ksplit_2", {"ksplit": (2, 0)}), ("ksplit_2_grid_7", {"ksplit": (2, 7)}),
    ("gn_a_0", {"gn_a": (0, 0)}), ("gn_a_2", {"gn_a": (2, 0)}),
    ("tile_2", {"tuning": (2, 0)}),
]

BATCHES, LATENTS = (2, 17), (64, 128)


def _unet(B, L):
    """SDXL UNet (block widths 320 / 640 / 1280, two resnets per level): conv1 of a resnet carries the time-embedding row vector,
    conv2 the residual; conv_in reads 4 channels padded to 8, conv_out writes 4."""
    rows = [("c3", B, L, L, 8, 320, {})]
    down = [(L, [(320, 320)], 320), (L // 2, [(320, 640), (640, 640)], 640), (L // 4, [(640, 1280), (1280, 1280)], None)]
    up = [(L // 4, [2560, 1920], 1280), (L // 2, [1920, 1280, 960], 640), (L, [960, 640], 320)]
    for s, pairs, ds in down:
        for cin, cout in pairs:
            rows += [("c3", B, s, s, cin, cout, {"rowvec": True}), ("c3", B, s, s, cout, cout, {"residual": True})]
        if ds:
            rows.append(("c3s2", B, s, s, ds, ds, {}))
    for s, cins, c in up:
        rows += [("c3", B, s, s, cin, c, {"rowvec": True}) for cin in cins] + [("c3", B, s, s, c, c, {"residual": True})]
        if s != L:
            rows += [("up2all", B, s, s, c, c, {}), ("up2par", B, s, s, c, c, {})]
    return rows + [("c3", B, L, L, 320, 4, {})]


def _vae(B, L):
    """VAE decoder (512, 512, 256, 128 from the latent up): fp32 residual stream, conv_out 128 -> 3 (padded to 4) in fp32."""
    rows = [("c3", B, L, L, 8, 512, {"flags": OUT_F32})]
    for s, pairs, upc in [(L, [(512, 512)], 512), (2 * L, [(512, 512)], 512), (4 * L, [(512, 256), (256, 256)], 256),
                          (8 * L, [(256, 128), (128, 128)], None)]:
        for cin, cout in pairs:
            rows += [("c3", B, s, s, cin, cout, {}), ("c3", B, s, s, cin, cout, {"flags": OUT_F32 | RES_F32, "residual": True})]
        if upc:
            rows += [("up2all", B, s, s, upc, upc, {}), ("up2all", B, s, s, upc, upc, {"flags": OUT_F32}),
                     ("up2par", B, s, s, upc, upc, {"flags": OUT_F32})]
    return rows + [("c3", B, 8 * L, 8 * L, 128, 4, {"flags": OUT_F32})]


def _tiny(B, L):
    """TAESDXL decoder and encoder: 64 -> 64 block convs with and without LB_GEMM_C64 at every level, the decoder's fused-upsample
    convs, the encoder's stride-2 convs, 8 -> 64 input convs and 64 -> 4 output convs."""
    rows = [("c3", B, L, L, 8, 64, {"flags": RELU}), ("c3", B, 8 * L, 8 * L, 8, 64, {}),
            ("c3", B, 8 * L, 8 * L, 64, 4, {}), ("c3", B, L, L, 64, 4, {})]
    for s in (L, 2 * L, 4 * L, 8 * L):
        rows += [("c3", B, s, s, 64, 64, {"flags": RELU}), ("c3", B, s, s, 64, 64, {"flags": RELU | C64}),
                 ("c3", B, s, s, 64, 64, {"flags": C64, "residual": True})]
        if s != 8 * L:
            rows += [("c3ups", B, s, s, 64, 64, {}), ("c3ups", B, s, s, 64, 64, {"flags": C64})]
        if s != L:
            rows.append(("c3s2", B, s, s, 64, 64, {}))
    return rows


# the non-square UNet levels of the table in native/geometry.py: (H, W, C, B)
NONSQUARE = [(96, 168, 320, 2), (48, 84, 640, 2), (24, 42, 1280, 2), (36, 64, 640, 2), (18, 32, 1280, 2), (28, 48, 640, 17),
             (14, 24, 1280, 17)]
# tests/test_halo_ksplit_cpu.py: SPLIT_SHAPES and WHOLE_ROUND_SHAPES
KSPLIT_SHAPES = [(17, 16, 16, 1280, 1280), (17, 32, 32, 640, 640), (17, 64, 64, 320, 320), (2, 64, 64, 320, 320),
                 (17, 64, 64, 512, 512), (17, 512, 512, 128, 128), (17, 128, 128, 512, 512)]
EDGES = [
    ("c3", 2, 64, 64, 64, 128, {}), ("c3", 17, 64, 64, 64, 128, {}), ("c3", 17, 64, 64, 128, 128, {}),       # Cin 64 and 128
    ("c3", 17, 64, 64, 128, 4, {}), ("c3", 17, 64, 64, 128, 16, {}), ("c3", 17, 64, 64, 128, 20, {}),        # N = 4 / 16 / 20
    ("c3", 17, 64, 64, 128, 4, {"residual": True}), ("c3", 2, 40, 24, 128, 4, {}),                          # N <= 16 outside the narrow kernel
    ("c3s2", 2, 32, 32, 320, 320, {}), ("c3ups", 2, 32, 32, 320, 320, {}),                                  # stride 2, ups = 1
    ("up2par", 17, 32, 32, 640, 640, {}), ("up2all", 17, 32, 32, 640, 640, {}), ("up2all", 1, 16, 16, 128, 128, {}),
    ("up2all", 2, 20, 24, 128, 128, {}),                                                                    # scatter 2 the halo kernel refuses
    ("c3", 17, 64, 64, 64, 64, {"flags": C64}), ("c3", 17, 64, 64, 128, 128, {"flags": C64}),               # C64: taken and refused
    ("c3", 17, 64, 64, 320, 320, {"zero_page": False}), ("c3", 2, 16, 16, 640, 320, {"partial": False}),
    ("c3", 2, 16, 16, 640, 320, {"partial": True}), ("c3", 1, 40, 24, 128, 128, {}), ("c3", 17, 520, 520, 128, 128, {}),
    ("c3", 17, 64, 64, 96, 128, {}),                                                                        # Cin % 64
    ("gemm", 4352, 0, 0, 1280, 1280, {"partial": False}), ("gemm", 4352, 0, 0, 1280, 1280, {"partial": True}),
    ("gemm", 512, 0, 0, 5120, 1280, {"partial": True}), ("gemm", 512, 0, 0, 1280, 1280, {"zero_page": False, "partial": True}),
    ("geglu", 4352, 0, 0, 1280, 10240, {"partial": False}), ("geglu", 4352, 0, 0, 1280, 10240, {"partial": True}),
    ("geglu", 512, 0, 0, 1280, 10240, {"zero_page": False}),
]


def rows():
    out = []
    for B in BATCHES:
        for L in LATENTS:
            out += _unet(B, L) + _vae(B, L) + _tiny(B, L)
    out += [("c3", B, H, W, C_, C_, {}) for H, W, C_, B in NONSQUARE]
    out += [("c3", B, H, W, cin, n, {}) for B, H, W, cin, n in KSPLIT_SHAPES]
    out += EDGES
    seen, uniq = set(), []
    for r in out:                       # (levels shared by two nets: once)
        key = (r[:6], tuple(sorted(r[6].items())))
        if key not in seen:
            seen.add(key)
            uniq.append(r)
    return uniq
