"""The bounds of the GEMM epilogue matrix (tests/test_gemm_epilogue_matrix_gpu.py) checked without a device: a plain fp32 emulation of
every epilogue, value kind and split count stays inside its bound at every element - the bounds admit a correct implementation - and
every mutant of tests/_gemm_epilogue_model.py puts at least one element outside it, in both value kinds - the bounds (and the chosen
shape and inputs) catch the ways an epilogue goes wrong.  Also here, because it returns before any device call: lb_gemm_f16's refusal
of LB_GEMM_TRANS_OUT | LB_GEMM_OUT_F32."""
import ctypes as C
import os

import pytest
import torch

import _gemm_epilogue_model as E
from _parity import check_elementwise, f64

KINDS = ["normal", "outliers"]


def _splits(epi):
    return [1] if E.EPILOGUES[epi].get("geglu") else [1, 2, 3]      # (a GEGLU launch is never split along K)


def test_flag_values_match_the_binding():
    from latentblending_amd.hip import lib
    assert (E.OUT_F32, E.RES_F32, E.GEGLU, E.TRANS_OUT, E.SILU, E.RELU, E.QUICK_GELU, E.GELU) == (
        lib.GEMM_OUT_F32, lib.GEMM_RES_F32, lib.GEMM_GEGLU, lib.GEMM_TRANS_OUT, lib.GEMM_SILU, lib.GEMM_RELU, lib.GEMM_QUICK_GELU, lib.GEMM_GELU)


def test_shape_has_the_edges_it_claims():
    assert all(E.M % h for h in (64, 128, 192, 256)) and E.N % 8 == 0 and E.N % 16 and E.K % 64 == 0 and (E.K // 64) % 2 == 1
    assert E.SAMPLES * E.ROWS_PER_SAMPLE == E.M and E.ROWS_PER_SAMPLE % 16
    assert E.k_slices(1) == [(0, 320)] and E.k_slices(2) == [(0, 192), (192, 320)] and E.k_slices(3) == [(0, 128), (128, 256), (256, 320)]


def _plan(k, flags):
    """lb_gemm_plan's (tile, splitk) for the matrix shape with K = ``k`` (host arithmetic: the pointers are never dereferenced)."""
    from latentblending_amd.hip import lib
    p = lib.gemm_params(A=4096, W=4096, C=4096, partial=4096, zero_page=64, M=E.M, N=E.N, K=k, lda=k, ldw=k, ldc=E.N, flags=flags)
    tile, sk = C.c_int(), C.c_int()
    lib.api.lb_gemm_plan(C.byref(p), C.byref(tile), C.byref(sk), None)
    return tile.value, sk.value


def test_every_forced_pair_of_the_matrix_is_planned_as_forced():
    """What the GPU file asserts before each launch, here without a device: at this shape every (variant, tile, splitk) of the matrix
    is the plan's answer - GEGLU excepted, which is never split - while an ineligible tile falls back silently: the reason for
    asking.  (Variant 1 is the library's default: lb_gemm_set_variant(1) itself sets kernel attributes on a device.)"""
    from latentblending_amd.hip import lib
    try:
        for variant, tile, splitk in E.UNSPLIT + E.SPLIT:
            lib.api.lb_gemm_set_variant(-1 if variant == 1 else 0, 0)
            lib.api.lb_gemm_set_tuning(tile, splitk)
            for epi in E.EPILOGUES:
                want = (tile, 1 if E.EPILOGUES[epi].get("geglu") else splitk)
                assert _plan(E.K, E.flags_of(epi)) == want, (variant, tile, splitk, epi)
        lib.api.lb_gemm_set_variant(-1, 0)
        lib.api.lb_gemm_set_tuning(9, 1)
        assert _plan(E.K + 8, 0)[0] != 9                 # K % 64 != 0: no ping-pong kernel, and nothing says so
        lib.api.lb_gemm_set_variant(0, 0)
        lib.api.lb_gemm_set_tuning(4, 1)
        assert _plan(E.K, 0)[0] == 1                     # the 8-wave tiles exist in the direct-to-LDS family only
    finally:
        lib.api.lb_gemm_set_tuning(0, 0)
        lib.api.lb_gemm_set_variant(-1, 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("epi", list(E.EPILOGUES))
def test_fp32_emulation_is_inside_every_bound(epi, kind):
    ref, bound = E.reference(kind, epi)
    log = {}
    for splits in _splits(epi):
        got = E.emulate(kind, epi, splits)
        assert got.dtype == (torch.float32 if E.EPILOGUES[epi].get("out_f32") else torch.float16) and got.shape == ref.shape
        check_elementwise(log, f"emu_{epi}_{kind}_sk{splits}", got, ref, bound)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mutant", list(E.MUTANTS))
def test_every_mutant_leaves_the_bound(mutant, kind):
    epi = E.MUTANTS[mutant]
    ref, bound = E.reference(kind, epi)
    for splits in _splits(epi):
        got = f64(E.emulate(kind, epi, splits, mutant=mutant))
        err = (got - ref).abs()
        bad = int((~(err <= bound)).sum())          # (a NaN - an element never stored - is outside)
        print(f"[mutant] {mutant} {kind} sk{splits}: {bad}/{err.numel()} elements outside the bound")
        assert bad >= 1, f"{mutant} ({kind}, {splits} slices) stays inside the bound of {epi!r} everywhere: the matrix would not notice it"


def test_rowvec_mutant_is_wrong_only_across_a_sample_boundary():
    """The shape's point: rows of one 16-row group lie in two samples, and only they tell the two index forms apart."""
    good, bad = E.emulate("normal", "bias_rv_res"), E.emulate("normal", "bias_rv_res", mutant="rowvec_index_of_tile_row")
    rows = torch.nonzero((good != bad).any(dim=1)).flatten().tolist()
    assert rows and all(m // 16 * 16 // E.ROWS_PER_SAMPLE != m // E.ROWS_PER_SAMPLE for m in rows)


def test_trans_out_with_out_f32_is_refused():
    """Every epilogue stores the transposed form as fp16 while the callers size an fp32 buffer for the pair: lb_gemm_f16 refuses it
    before routing, names both flags, and leaves the output alone.  (Host memory throughout: nothing is launched.)"""
    from latentblending_amd.hip import lib
    M, N, K = 64, 64, 64
    a, w = (C.c_uint16 * (M * K))(), (C.c_uint16 * (N * K))()
    out = (C.c_uint8 * (M * N * 4))(*([0xA5] * (M * N * 4)))
    for extra in (0, lib.GEMM_RES_F32, lib.GEMM_RELU):
        p = lib.gemm_params(A=C.addressof(a), W=C.addressof(w), C=C.addressof(out), M=M, N=N, K=K, lda=K, ldw=K, ldc=M,
                            flags=lib.GEMM_TRANS_OUT | lib.GEMM_OUT_F32 | extra)
        with pytest.raises(RuntimeError) as ei:
            lib.api.lb_gemm_f16(C.byref(p), None)
        assert "LB_GEMM_TRANS_OUT" in str(ei.value) and "LB_GEMM_OUT_F32" in str(ei.value)
    assert bytes(out) == b"\xa5" * (M * N * 4)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "lb_hip.h")) as fh:
        line = next(ln for ln in fh if "LB_GEMM_TRANS_OUT = 8" in ln)
    assert "fp16 only" in line
