"""The epilogue of lb_gemm_f16 on the CPU, written once for tests/test_gemm_epilogue_matrix_cpu.py and ..._gpu.py:

  * ``matrix_case``  the seeded operands of one value kind at the one shape of the matrix, with their float64 products;
  * ``reference``    the float64 result of every epilogue of EPILOGUES and its derived per-element bound (tests/_parity.py);
  * ``emulate``      a plain fp32 emulation of what a correct kernel does - fp16 operands, fp32 products per K slice, the slices summed
                     in slice order, then alpha, bias, row vector, residual, activation and the store rounding in the order of
                     lb_gemm_store4 (csrc/lb_gemm.h) - and, on request, of one of the MUTANTS: the ways such an epilogue goes wrong.

The CPU test shows that the bounds admit the emulation and reject every mutant; the GPU test holds the kernels to the same bounds."""
import functools

import torch
import torch.nn.functional as F

from _parity import absdot, accumulate_bound, activation_bound, contraction_bound, epilogue_bound, geglu_bound, rnd
from _value_kinds import outliers, tame_outlier_weights

F16, F32, F64 = torch.float16, torch.float32, torch.float64

# M is ragged for every tile height (64, 128, 192, 256); N is a multiple of 8 (GEGLU) but not of 16, so a 16-column group straddles N
# and the last wave tile overhangs; K = 5 K-tiles of 64 (an odd count for the ping-pong kernel, no even division into 2 or 3 slices);
# 4 samples of 150 rows for the row vector: 150 is no multiple of 16, so wave tiles of every tile shape cross a sample boundary.
M, N, K = 600, 392, 320
SAMPLES, ROWS_PER_SAMPLE = 4, 150
BK = 64

# (variant, tile, splitk) of the matrix: variant 1 = the direct-to-LDS family (and the ping-pong kernel, tile 9), 0 = the register ring
UNSPLIT = [(1, t, 1) for t in (1, 2, 3, 4, 5, 7, 9, 10, 11)] + [(0, t, 1) for t in (1, 2, 3)]
SPLIT = [(1, t, s) for t, s in ((3, 2), (3, 3), (1, 3), (2, 2), (4, 3), (10, 2), (9, 3), (11, 2))] + [(0, 3, 3), (0, 1, 2)]

# include/lb_hip.h (the CPU test compares them with the binding's)
OUT_F32, RES_F32, GEGLU, TRANS_OUT, SILU, RELU, QUICK_GELU, GELU = 1, 2, 4, 8, 16, 32, 128, 256

# name -> what the epilogue does; keys: alpha, bias, rowvec, res ("f16" | "f32"), act, out_f32, trans, geglu
EPILOGUES = {
    "none": dict(),
    "bias_rv_res": dict(bias=True, rowvec=True, res="f16"),
    "alpha": dict(alpha=2.0 ** -3, bias=True, res="f16"),
    "f32": dict(alpha=2.0 ** -3, bias=True, res="f32", out_f32=True),
    "outf32_res16": dict(res="f16", out_f32=True),
    "silu": dict(bias=True, rowvec=True, res="f16", act="silu"),
    "relu": dict(bias=True, res="f16", act="relu"),
    "relu_f32": dict(bias=True, res="f32", out_f32=True, act="relu"),
    "quick_gelu": dict(bias=True, act="quick_gelu"),
    "gelu": dict(bias=True, act="gelu"),
    "trans": dict(bias=True, res="f16", trans=True),
    "geglu": dict(bias=True, geglu=True),
}
_ACT_FLAG = {"silu": SILU, "relu": RELU, "quick_gelu": QUICK_GELU, "gelu": GELU}

# mutant -> the epilogue it is planted in
MUTANTS = {
    "rowvec_index_of_tile_row": "bias_rv_res",      # sample index from the wave tile's first row: wrong only across a sample boundary
    "activation_before_residual": "silu",
    "alpha_on_bias": "alpha",
    "residual_row_stride": "bias_rv_res",           # the residual's rows read ldr + 4 apart
    "res_f32_read_as_f16": "f32",
    "slice_dropped": "bias_rv_res",
    "slice_twice": "bias_rv_res",
    "trans_quad_swapped": "trans",                  # (m, n) exchanged inside a 4 x 4 block of the transposed store
    "last_quad_skipped": "bias_rv_res",             # columns N - 4 .. N - 1 never stored
    "gelu_as_quick_gelu": "gelu",
    "geglu_halves_swapped": "geglu",
}


def flags_of(epi):
    e = EPILOGUES[epi]
    return ((OUT_F32 if e.get("out_f32") else 0) | (RES_F32 if e.get("res") == "f32" else 0) | (GEGLU if e.get("geglu") else 0) |
            (TRANS_OUT if e.get("trans") else 0) | _ACT_FLAG.get(e.get("act"), 0))


@functools.lru_cache(maxsize=None)
def matrix_case(kind):
    """Operands (fp16 / fp32 on the CPU) and the float64 products of one value kind: computed once, shared, never modified."""
    if kind == "normal":
        A, W = rnd(M, K, seed=701), rnd(N, K, seed=702, scale=K ** -0.5)
    elif kind == "outliers":
        A, W = outliers((M, K), 703), tame_outlier_weights(rnd(N, K, seed=704, scale=K ** -0.5))
    else:
        raise KeyError(kind)
    A64, W64 = A.double(), W.double()
    return dict(A=A, W=W, bias=rnd(N, seed=705, dtype=F32), res=rnd(M, N, seed=706), rv=rnd(SAMPLES, N, seed=707),
                res32=rnd(M, N, seed=708, dtype=F32, scale=100.0), base=A64 @ W64.t(), ad=absdot(A64, W64))


def operands(case, epi):
    """(bias, rowvec, residual) tensors of ``epi`` (None where it has none)."""
    e = EPILOGUES[epi]
    res = {None: None, "f16": case["res"], "f32": case["res32"]}[e.get("res")]
    return (case["bias"] if e.get("bias") else None), (case["rv"] if e.get("rowvec") else None), res


def _act64(name, y):
    return {"silu": F.silu, "relu": F.relu, "quick_gelu": lambda t: t * torch.sigmoid(1.702 * t), "gelu": F.gelu}[name](y)


@functools.lru_cache(maxsize=None)
def reference(kind, epi):
    """(float64 reference, per-element bound) of ``epi`` in the layout of the output: [M, N], [N, M] (trans) or [M, N / 2] (GEGLU)."""
    c, e = matrix_case(kind), EPILOGUES[epi]
    alpha, out_f32 = e.get("alpha", 1.0), bool(e.get("out_f32"))
    bias, rv, res = operands(c, epi)
    rows = None if rv is None else rv.double().repeat_interleave(ROWS_PER_SAMPLE, 0)
    y = alpha * c["base"]
    for t in (bias, rows, res):
        if t is not None:
            y = y + t.double()
    if e.get("geglu"):
        pre = accumulate_bound(c["ad"], K, alpha) + epilogue_bound(y, bias)
        (h, gt), (ph, pg) = y.chunk(2, dim=-1), pre.chunk(2, dim=-1)
        return h * F.gelu(gt), geglu_bound(ph, pg, h, gt, F.gelu(gt))
    if e.get("act"):
        ref = _act64(e["act"], y)
        bound = activation_bound(accumulate_bound(c["ad"], K, alpha) + epilogue_bound(y, bias, res, rows), ref, out_f32=out_f32)
    else:
        ref = y
        bound = contraction_bound(None, None, K, y, out_f32=out_f32, alpha=alpha, bias=bias, residual=res, rowvec=rows, absdot64=c["ad"])
    if e.get("trans"):
        ref, bound = ref.t().contiguous(), bound.t().contiguous()
    return ref, bound


def k_slices(splits):
    """The K ranges of the kernels' split-K slices: ceil(K tiles / splits) 64-wide tiles each, the last one shorter."""
    tiles = (K + BK - 1) // BK
    per = (tiles + splits - 1) // splits
    return [(z * per * BK, min((z + 1) * per * BK, K)) for z in range(splits) if z * per * BK < K]


def _act32(name, o):
    one = torch.ones((), dtype=F32)
    if name == "silu":
        return o * (one / (one + torch.exp(-o)))
    if name == "relu":
        return torch.clamp_min(o, 0.0)
    if name == "quick_gelu":
        return o * (one / (one + torch.exp(o * -1.702)))
    return 0.5 * o * (one + torch.erf(o * 0.70710678118654752440))


def emulate(kind, epi, splits=1, mutant=None):
    """The output an fp32 implementation of ``epi`` stores (its dtype and layout), NaN where it stores nothing.  ``mutant``: one of
    MUTANTS, planted in this run."""
    assert mutant is None or MUTANTS[mutant] == epi, (mutant, epi)
    c, e = matrix_case(kind), EPILOGUES[epi]
    alpha, out_f32 = torch.tensor(e.get("alpha", 1.0), dtype=F32), bool(e.get("out_f32"))
    bias, rv, res = operands(c, epi)
    A32, W32 = c["A"].float(), c["W"].float()
    # a dropped / doubled slice of an unsplit launch is one of its K-tiles
    slices = k_slices(splits if splits > 1 or mutant not in ("slice_dropped", "slice_twice") else (K + BK - 1) // BK)
    acc = torch.zeros(M, N, dtype=F32)
    for z, (k0, k1) in enumerate(slices):
        part = A32[:, k0:k1] @ W32[:, k0:k1].t()
        if z == 1 and mutant == "slice_dropped":
            continue
        acc = acc + part
        if z == 1 and mutant == "slice_twice":
            acc = acc + part
    if e.get("geglu"):
        half = N // 2
        y = acc * alpha + bias[None, :]
        h, gt = (y[:, half:], y[:, :half]) if mutant == "geglu_halves_swapped" else (y[:, :half], y[:, half:])
        return (h * _act32("gelu", gt)).to(F16)
    o = acc * alpha
    if bias is not None:
        o = (acc + bias[None, :]) * alpha if mutant == "alpha_on_bias" else o + bias[None, :]
    if rv is not None:
        m = torch.arange(M)
        idx = (m // 16 * 16 if mutant == "rowvec_index_of_tile_row" else m) // ROWS_PER_SAMPLE
        o = o + rv.float()[idx]
    act = e.get("act")
    if mutant == "gelu_as_quick_gelu":
        act = "quick_gelu"
    if mutant == "activation_before_residual":
        o, act = _act32(act, o), None
    if res is not None:
        r = res
        if mutant == "residual_row_stride":
            flat = torch.arange(M)[:, None] * (N + 4) + torch.arange(N)[None, :]
            r = res.reshape(-1)[flat % res.numel()]
        if mutant == "res_f32_read_as_f16":
            r = r.to(F16)
        o = o + r.float()
    if act:
        o = _act32(act, o)
    o = o if out_f32 else o.to(F16)
    if mutant == "last_quad_skipped":
        o[:, N - 4:] = float("nan")
    if e.get("trans"):
        if mutant == "trans_quad_swapped":
            o = o.reshape(M // 4, 4, N // 4, 4).transpose(1, 3).reshape(M, N)
        o = o.t().contiguous()
    return o
