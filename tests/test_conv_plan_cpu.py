"""How a conv is routed and planned, held to answers FROZEN at the commit before the routing was gathered into one function.

tests/golden/conv_plan_parent.json holds what the six plan exports of that commit - lb_gemm_plan, lb_conv_halo_plan,
lb_gemm_ch_stat_rows, lb_conv_halo_ksplit_plan, lb_conv_halo_ksplit_workspace_bytes, lb_conv_halo_gn_a_plan - answered for every
row of tests/_conv_plan_grid.py under every flag set and switch setting there (recorded with 256 CUs: the count the library
assumes without a device, and the MI355X's).  Here the same six exports must reproduce it exactly, and every field of lb_conv_plan
must equal the same recorded values: the exports are thin reads of the code behind lb_conv_plan, so comparing them with each other
in one build would only be the code under test checking itself."""
import ctypes as C
import json
import os

import pytest

import _conv_plan_grid as G
from latentblending_amd.hip import lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_parent.json")
COLUMNS = ["plan_refused", "tile", "splitk", "blocks", "halo_kind", "halo_tile_w", "halo_items", "halo_grid", "stat_rows",
           "ksplit_units", "ksplit_grid", "ksplit_split", "ksplit_workspace_bytes", "gn_a_fuse", "gn_a_kind"]
SLAB_BYTES = 256 * 128 * 4


def build_params(row, flags):
    kind, B, H, W, cin, cout, opt = row
    flags |= opt.get("flags", 0)
    if kind in ("gemm", "geglu"):
        n_out = cout // 2 if kind == "geglu" else cout
        flags |= G.GEGLU if kind == "geglu" else 0
        shape = dict(M=B, N=cout, K=cin, lda=cin, ldw=cin, ldc=n_out, ldr=n_out)
    else:
        ks, stride, pad, ups, scatter = G.KINDS[kind]
        g = lib.ConvGeom(H, W, cin, ks, ks, stride=stride, pad=pad, ups=ups, parity=[None, (0, 0), "all"][scatter])
        shape = dict(M=g.M(B), N=cout, K=g.K, ldw=g.K, ldc=cout, ldr=cout, conv=g)
    M = shape["M"]
    small = ((M + 63) // 64) * ((cout + 63) // 64) <= 640 and kind != "geglu"
    fake = lambda on: 4096 if on else None      # noqa: E731  (host arithmetic only: never dereferenced)
    return lib.gemm_params(A=4096, W=4096, C=4096, residual=fake(opt.get("residual")), rowvec=fake(opt.get("rowvec")), ld_rowvec=cout,
                           rows_per_batch=M // B, partial=fake(opt.get("partial", small)), flags=flags,
                           zero_page=64 if opt.get("zero_page", True) else None, **shape)


def old_exports(api, p):
    """The six exports' answers for ``p``, in the order of COLUMNS (``api``: raw or bound functions of either commit)."""
    tile, sk, nb = C.c_int(), C.c_int(), C.c_long()
    try:
        refused = int(bool(api.lb_gemm_plan(C.byref(p), C.byref(tile), C.byref(sk), C.byref(nb))))
    except RuntimeError:
        refused = 1
    kind, tw, items, grid = C.c_int(), C.c_int(), C.c_long(), C.c_long()
    api.lb_conv_halo_plan(C.byref(p), C.byref(kind), C.byref(tw), C.byref(items), C.byref(grid))
    units, kgrid, split = C.c_long(), C.c_long(), C.c_int()
    api.lb_conv_halo_ksplit_plan(C.byref(p), C.byref(units), C.byref(kgrid), C.byref(split))
    fuse, gkind = C.c_int(), C.c_int()
    api.lb_conv_halo_gn_a_plan(C.byref(p), C.byref(fuse), C.byref(gkind))
    return [refused, tile.value, sk.value, nb.value, kind.value, tw.value, items.value, grid.value,
            int(api.lb_gemm_ch_stat_rows(C.byref(p))), units.value, kgrid.value, split.value,
            int(api.lb_conv_halo_ksplit_workspace_bytes(C.byref(p))), fuse.value, gkind.value]


def grid_signature():
    """The grid as the fixture echoes it: a fixture recorded for another grid is refused, not misread."""
    return json.loads(json.dumps([list(r[:6]) + [sorted(r[6].items())] for r in G.rows()]))


def apply_setting(api, overrides):
    s = dict(G.DEFAULTS, **overrides)
    api.lb_gemm_set_halo(s["halo"])
    api.lb_conv_halo_set_ksplit(*s["ksplit"])
    api.lb_conv_halo_set_gn_a(*s["gn_a"])
    api.lb_gemm_set_tuning(*s["tuning"])


@pytest.fixture(scope="module")
def frozen():
    with open(FIXTURE) as fh:
        fx = json.load(fh)
    assert fx["compute_units"] == 256 and fx["columns"] == COLUMNS
    assert fx["flag_sets"] == G.FLAG_SETS and fx["settings"] == [n for n, _ in G.SETTINGS]
    assert fx["rows"] == grid_signature(), "the grid moved: the fixture must be recorded again at the commit it freezes"
    return fx


def test_flag_bits_of_the_grid_are_the_librarys():
    assert (G.OUT_F32, G.RES_F32, G.GEGLU, G.RELU) == (lib.GEMM_OUT_F32, lib.GEMM_RES_F32, lib.GEMM_GEGLU, lib.GEMM_RELU)
    assert (G.RAGGED, G.C64, G.KSPLIT, G.GN_A) == (lib.GEMM_HALO_RAGGED, lib.GEMM_C64, lib.GEMM_HALO_KSPLIT, lib.GEMM_GN_A)


@pytest.mark.parametrize("si", range(len(G.SETTINGS)), ids=[n for n, _ in G.SETTINGS])
def test_exports_and_conv_plan_give_the_frozen_answers(si, frozen):
    api, conv_plan = lib.api, lib._lib.lb_conv_plan         # (unchecked: a refusal is an answer here)
    answers, nf, ns = frozen["answers"], len(G.FLAG_SETS), len(G.SETTINGS)
    col = {c: i for i, c in enumerate(COLUMNS)}
    apply_setting(api, G.SETTINGS[si][1])
    try:
        for ri, row in enumerate(G.rows()):
            want_by_flag = [answers[frozen["index"][ri][fi * ns + si]] for fi in range(nf)]
            for fi, flags in enumerate(G.FLAG_SETS):
                p, want, where = build_params(row, flags), want_by_flag[fi], (G.SETTINGS[si][0], row, flags)
                assert old_exports(api, p) == want, where
                plan = lib.LbConvPlan()
                rc = conv_plan(C.byref(p), C.byref(plan))
                w = lambda c: want[col[c]]      # noqa: E731
                assert int(bool(rc)) == w("plan_refused"), where
                assert (plan.tile, plan.splitk, plan.blocks) == (w("tile"), w("splitk"), w("blocks")), where
                assert (plan.halo_kind, plan.halo_tile_w, plan.halo_items, plan.halo_grid) == \
                    (w("halo_kind"), w("halo_tile_w"), w("halo_items"), w("halo_grid")), where
                assert plan.stat_rows == w("stat_rows"), where
                assert (plan.ksplit_units, plan.ksplit_grid, plan.ksplit_split) == (w("ksplit_units"), w("ksplit_grid"), w("ksplit_split")), where
                assert plan.ksplit_counter_bytes + plan.ksplit_slab_bytes == w("ksplit_workspace_bytes"), where
                assert plan.ksplit_slab_bytes == (2 * w("ksplit_grid") * SLAB_BYTES if w("ksplit_split") else 0), where
                assert (plan.gn_a_fuse, plan.gn_a_kind) == (w("gn_a_fuse"), w("gn_a_kind")), where
                # the route: what the tile codes of the old plan name, and the one launch they never named (scatter = 2)
                if p.flags & G.C64:
                    want_route = lib.ROUTE_C64                   # (taken or refused: never another route)
                elif p.scatter == 2:
                    want_route = lib.ROUTE_UPCONV_HALO
                else:
                    want_route = {8: lib.ROUTE_NARROW, 6: lib.ROUTE_HALO3}.get(w("tile"), lib.ROUTE_GEMM)
                assert plan.route == want_route and (w("tile") == 12) == (want_route == lib.ROUTE_C64 and not rc), where
                # the ragged alternative of an unflagged conv the whole-tile form refuses = the frozen answer WITH the flag
                if not flags & G.RAGGED and w("halo_kind") == 0:
                    alt = want_by_flag[G.FLAG_SETS.index(flags | G.RAGGED)] if (flags | G.RAGGED) in G.FLAG_SETS else None
                    if alt is not None:
                        assert (plan.ragged_kind, plan.ragged_tile_w) == (alt[col["halo_kind"]], alt[col["halo_tile_w"]]), where
                else:
                    assert (plan.ragged_kind, plan.ragged_tile_w) == (0, 0), where
    finally:
        apply_setting(api, {})


# ---------------------------------------------------------------- the emitter's probes
def _upconv_levels():
    """(B, H, W, c) of every upsampler conv the UNet and VAE builders pass to Emitter.upconv_one_launch: the UNet's two lower levels
    (square latents 64 / 128 and the non-square renders of native/geometry.py's table, 1280 and 640 channels), the VAE decoder's
    three (512, 512, 256 channels at 1x, 2x, 4x the latent)."""
    latents = [(L, L) for L in G.LATENTS] + [(96, 168), (72, 128), (56, 96)]
    for B in (1,) + G.BATCHES:
        for H, W in latents:
            yield from [(B, H // 4, W // 4, 1280), (B, H // 2, W // 2, 640)]
            yield from [(B, H, W, 512), (B, 2 * H, 2 * W, 512), (B, 4 * H, 4 * W, 256)]


def test_upconv_one_launch_agrees_with_its_former_shape_arithmetic():
    """Emitter.upconv_one_launch asks lb_conv_plan whether the halo kernel takes the conv; until then it restated
    lb_upconv_halo_eligible in Python.  On every level the builders pass, the two agree."""
    from latentblending_amd.native.runtime import Emitter
    answers = set()
    for B, H, W, c in _upconv_levels():
        shape_ok = c % 64 == 0 and ((W % 32 == 0 and H % 8 == 0) or (W % 16 == 0 and H % 16 == 0))
        former = shape_ok and B * (H * W // 256) * 4 * ((c + 127) // 128) >= 96
        assert Emitter.upconv_one_launch(B, H, W, c, c) == former, (B, H, W, c)
        answers.add((shape_ok, former))
    assert answers == {(True, True), (True, False), (False, False)}      # (every branch of the rule is among the levels)


def test_probes_plan_without_allocating(monkeypatch):
    """halo_stat_rows and gn_operand plan through the record alone: no split-K and no K-split workspace appears for a probe."""
    import torch
    import latentblending_amd.native.runtime as rt
    monkeypatch.setattr(rt, "_stream", lambda: None)
    em = rt.Emitter(rt.Arena("cpu"))
    assert em.halo_stat_rows(17, 64, 64, 320, 320) > 0 and em.halo_stat_rows(2, 16, 16, 640, 320) == 0
    B, H, Cin, N = 17, 64, 320, 320                       # a conv the default policy splits along K: no fold, a GroupNorm launch
    x, w = torch.empty(B, H, H, Cin, dtype=torch.float16), torch.empty(N, 9 * Cin, dtype=torch.float16)
    gamma, st = torch.ones(Cin), (torch.zeros(Cin, B * 4, 2), 4)
    conv = lib.ConvGeom.conv3x3(H, H, Cin)
    prog = rt.Program("t")
    with prog.record():
        g = em.gn_operand(x, w, M=B * H * H, conv=conv, gamma=gamma, beta=gamma, B=B, HW=H * H, C_=Cin, eps=1e-6, silu=True, groups=32,
                          ch_stats=st)
        assert g.table is None and em.ws_gemm is None and em.ws_ksplit is None
        em.gemm(x, w, torch.empty(B * H * H, N, dtype=torch.float16), M=B * H * H, conv=conv, gn=g)
    assert em.ws_ksplit is not None and prog.op_names() == ["lb_groupnorm_from_stats", "lb_conv3x3_halo_f16"]
