"""The CLIP text towers and the LPIPS-Alex metric, unit by unit, at the shapes production runs (a real MI355X).

CLIP (``_CLIPProgram.marks``): one prompt is M = 77 rows at widths 768 and 1280, with the empty prompt (EOS at 1: the negative prompt of
every guided render), a short one (EOS at 9) and a truncated one (EOS at 76); M = 154 next to it, and a narrow tower whose residual
stream carries the "massive activations" of trained towers.  Per case: the route census (marks, ops, the plan of every launched GEMM),
every unit teacher-forced against float64 within ``FACTOR`` x the storage model (tests/_text_lpips_units.py), penultimate and pooled
against a free-running float64 forward, replays (eager, repeated, as a graph) bit for bit, and the arena lifetimes under NaN poison.

LPIPS (``NativeLPIPS``): smooth frames and transition-like neighbours instead of white noise, at sizes where the five convs leave
tile 3 and split along K; every conv teacher-forced against float64, the distance kernel against the float64 formula on the native
taps within a derived fp32 bound, free-running distances against float64 from the uint8 frames by groups of pairs, and the exact
properties the blending engine relies on: d(a, a) = 0, symmetry, independence from slot and chunk, a re-zeroed accumulator.
"""
import contextlib
import functools
import time
import types

import pytest
import torch

import _model_units as MU
import _text_lpips_units as TL
from oracle import sdxl_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, F32, F64 = torch.float16, torch.float32, torch.float64

BASE = dict(vocab_size=1000, bos_token_id=998, eos_token_id=999, num_hidden_layers=3)
CLIP_CASES = {
    "clip_l_B1": dict(cfg=dict(BASE, hidden_size=768, num_attention_heads=12, intermediate_size=3072, hidden_act="quick_gelu",
                               projection_dim=None, pad_token_id=999), B=1, prompts=((1,), (9,), (76,))),
    "bigg_B1": dict(cfg=dict(BASE, hidden_size=1280, num_attention_heads=20, intermediate_size=5120, hidden_act="gelu",
                             projection_dim=1280, pad_token_id=0), B=1, prompts=((1,), (9,), (76,))),
    "bigg_B2": dict(cfg=dict(BASE, hidden_size=1280, num_attention_heads=20, intermediate_size=5120, hidden_act="gelu",
                             projection_dim=1280, pad_token_id=0), B=2, prompts=((1, 76),)),
    "tiny_B3_hot": dict(cfg=dict(BASE, hidden_size=128, num_attention_heads=2, intermediate_size=256, hidden_act="gelu",
                                 projection_dim=64, pad_token_id=1), B=3, prompts=((1, 40, 76),), hot=True),
}
LPIPS_CASES = {
    "batch4_515": dict(N=4, H=515, W=515),
    "single_259x291": dict(N=1, H=259, W=291),
    "single_1024": dict(N=1, H=1024, W=1024),
}


def native():
    import latentblending_amd.native as n
    return n


def lib():
    from latentblending_amd.hip import lib as l
    return l


def lifetimes():
    import test_model_units_gpu as G        # ``check_lifetimes``: the poisoned replay of the UNet / VAE unit suite, not a copy of it
    return G.check_lifetimes


@contextlib.contextmanager
def gemm_census(log):
    """While active, every lb_gemm_f16 call (recorded or launched) appends the library's plan for the very parameter block it was
    handed: the ``lb_gemm_f16`` attribute of the ``api`` object is wrapped, the emitter is not touched."""
    l = lib()
    real = l.api.lb_gemm_f16

    def counted(pref, stream):
        p = pref._obj
        plan = l.conv_plan(p)
        log.append(dict(M=p.M, N=p.N, K=p.K, conv=int(p.conv), flags=int(p.flags), ws=bool(p.partial), route=int(plan.route),
                        tile=int(plan.tile), splitk=int(plan.splitk), blocks=int(plan.blocks)))
        return real(pref, stream)
    l.api.lb_gemm_f16 = counted
    try:
        yield log
    finally:
        l.api.lb_gemm_f16 = real


# ---------------------------------------------------------------------------------------------------------------- CLIP cases
def clip_cfg(case):
    return native().CLIPTextConfig(**CLIP_CASES[case]["cfg"])


@functools.lru_cache(maxsize=None)
def clip_case(case):
    """Build (journal on, census on), run every prompt once through the ONE program, capture after each: what the tests share."""
    n, c, cfg = native(), CLIP_CASES[case], clip_cfg(case)
    w = TL.clip_weights(cfg, 3)
    if c.get("hot"):
        w = TL.make_hot(w, cfg)
    tower = n.NativeCLIPText(cfg, n.DictProvider(w), DEV)
    plans = []
    with gemm_census(plans):
        prog = tower.build(c["B"], journal=True)
    ref, model = MU.evs(w)
    runs = []
    for eos_at in c["prompts"]:
        ids = TL.make_ids(cfg, eos_at, seed=11 + sum(eos_at))
        pen, pooled = prog.run(ids)
        torch.cuda.synchronize()
        pen, pooled = pen.clone(), None if pooled is None else pooled.clone()
        taps = {k: v.cpu() for k, v in prog.capture().items()}
        torch.cuda.synchronize()
        after = (prog.penultimate.clone(), None if prog.pooled is None else prog.pooled.clone())
        runs.append(types.SimpleNamespace(eos_at=eos_at, ids=ids, pen=pen, pooled=pooled, taps=taps, after=after))
    return types.SimpleNamespace(case=case, c=c, cfg=cfg, tower=tower, prog=prog, plans=plans, ref=ref, model=model, runs=runs)


def _key(case, run):
    return f"units_clip_{case}/eos" + "_".join(str(e) for e in run.eos_at)


@pytest.mark.parametrize("case", list(CLIP_CASES))
def test_clip_routes_marks_and_capture(case, results_log):
    s = clip_case(case)
    cfg, B = s.cfg, s.c["B"]
    units = TL.clip_units(cfg)
    assert [(m.name, m.kind, m.inputs) for m in s.prog.marks] == units
    MU.check_marks(s.prog.marks, {s.prog.prog.name: s.prog.prog}, ("ids",))
    names = s.prog.prog.op_names()
    L = cfg.num_hidden_layers
    assert names.count("lb_attn_fwd_d64") == L and names.count("lb_layernorm_f16") == 2 * L + (1 if cfg.projection_dim else 0)
    assert s.tower.build(B).prog.op_names() == names                    # the journal and the marks change no op
    # the census: 4 GEMMs per layer (+ the projection), in emission order, with the plan of the block that was launched
    want = [(B * 77, nn, kk) for _ in range(L) for nn, kk in ((3 * cfg.hidden_size, cfg.hidden_size), (cfg.hidden_size, cfg.hidden_size),
                                                              (cfg.intermediate_size, cfg.hidden_size), (cfg.hidden_size, cfg.intermediate_size))]
    if cfg.projection_dim:
        want.append((B, cfg.projection_dim, cfg.hidden_size))
    assert [(p["M"], p["N"], p["K"]) for p in s.plans] == want
    assert all(p["route"] == lib().ROUTE_GEMM and p["tile"] >= 1 and p["splitk"] >= 1 for p in s.plans)
    results_log[f"units_clip_{case}/census"] = s.plans[:4] + s.plans[4 * L:]
    print(f"[units] {case} census: " + " ".join(f"{p['M']}x{p['N']}x{p['K']}:t{p['tile']}k{p['splitk']}" for p in s.plans[:4] + s.plans[4 * L:]))
    for r in s.runs:        # a capture is a replay: it leaves the outputs as the launch did, and its taps are the outputs
        assert set(r.taps) == {u[0] for u in units}
        assert torch.equal(r.after[0], r.pen) and torch.equal(r.taps["penultimate"], r.pen.cpu())
        if cfg.projection_dim:
            assert torch.equal(r.after[1], r.pooled) and torch.equal(r.taps["pooled"], r.pooled.cpu())
        assert all(torch.isfinite(t.float()).all() for t in r.taps.values())


def test_clip_one_prompt_is_planned_unlike_two():
    """The B = 1 cases exist because M = 77 is planned differently from M = 154: at least one of the four layer GEMMs of the wide
    tower gets another (tile, split-K).  If every plan were shared, B = 1 would add nothing and the case list would have to change."""
    one, two = clip_case("bigg_B1").plans[:4], clip_case("bigg_B2").plans[:4]
    assert [(p["N"], p["K"]) for p in one] == [(p["N"], p["K"]) for p in two]
    assert [(p["tile"], p["splitk"]) for p in one] != [(p["tile"], p["splitk"]) for p in two], (one, two)


def _clip_unit_params():
    out = []
    for case, c in CLIP_CASES.items():
        for ri, eos_at in enumerate(c["prompts"]):
            for name, kind, ins in TL.clip_units(types.SimpleNamespace(**c["cfg"])):
                out.append(pytest.param(case, ri, name, kind, ins, id=f"{case}-eos{'_'.join(map(str, eos_at))}-{name}"))
    return out


@pytest.mark.parametrize("case,ri,name,kind,ins", _clip_unit_params())
def test_clip_unit_matches_fp64(case, ri, name, kind, ins, results_log):
    """Teacher-forced: the unit in float64 on the NATIVE inputs of that unit.  ``penultimate`` is a copy: the same bits as the input
    of the last layer.  ``pooled`` gathers its row by transformers' rule in the reference: a wrong row fails by orders of magnitude.
    A quick-GELU fc1 is also held to its constant (``quick_gelu_fit``): 1.7 for 1.702 hides inside an fp16 rounding element by element."""
    s = clip_case(case)
    r = s.runs[ri]
    given = [r.ids if i == "ids" else r.taps[i] for i in ins]
    if kind == "penultimate":
        assert torch.equal(r.taps[name].reshape(given[0].shape), given[0])
        return
    ref64 = TL.clip_unit(s.ref, s.cfg, name, kind, given)
    model = TL.clip_unit(s.model, s.cfg, name, kind, given)
    bad = MU.compare(results_log, f"{_key(case, r)}/{name}", r.taps[name], model, ref64)
    assert bad is None, bad
    if kind == "fc1" and s.cfg.hidden_act == "quick_gelu":
        i = int(name[1:name.index(".")])
        e_rms = MU.FACTOR * float((model.double() - ref64).pow(2).mean().sqrt())
        dk, bound = TL.quick_gelu_fit(r.taps[name], TL.fc1_pre(s.ref, s.cfg, i, given[0]), e_rms)
        results_log[f"{_key(case, r)}/{name}/quick_gelu_constant"] = {"shift": dk, "bound": bound}
        print(f"[units] {_key(case, r)}/{name}: fitted quick-GELU constant 1.702 {dk:+.2e} (bound {bound:.2e})")
        assert abs(dk) <= bound, (dk, bound)


@pytest.mark.parametrize("case", list(CLIP_CASES))
def test_clip_free_running(case, results_log):
    """Penultimate and pooled against a float64 forward from the ids, within FACTOR x the free-running storage model: a hand-over
    between units that is consistent but wrong cannot pass this one."""
    s = clip_case(case)
    fails = []
    for r in s.runs:
        ref, model = TL.clip_forward(s.ref, s.cfg, r.ids), TL.clip_forward(s.model, s.cfg, r.ids)
        fails.append(MU.compare(results_log, f"{_key(case, r)}/free_running/penultimate", r.pen, model["penultimate"], ref["penultimate"]))
        if s.cfg.projection_dim:
            fails.append(MU.compare(results_log, f"{_key(case, r)}/free_running/pooled", r.pooled, model["pooled"], ref["pooled"]))
    fails = [f for f in fails if f]
    assert not fails, fails


@pytest.mark.parametrize("case", list(CLIP_CASES))
def test_clip_replay(case):
    """All prompts went through one program; the first again gives its first bits, and so does the instantiated graph."""
    s = clip_case(case)
    first = s.runs[0]

    def same():
        pen, pooled = s.prog.run(first.ids)
        torch.cuda.synchronize()
        return torch.equal(pen, first.pen) and (pooled is None or torch.equal(pooled, first.pooled))
    assert same()
    if len(s.runs) > 1:
        pen, _ = s.prog.run(s.runs[-1].ids)
        torch.cuda.synchronize()
        assert torch.equal(pen, s.runs[-1].pen) and not torch.equal(pen, first.pen)
    s.prog.prog.instantiate()
    assert s.prog.prog.graph_ready and same() and same()


@pytest.mark.parametrize("case", list(CLIP_CASES))
def test_clip_reads_no_free_buffer(case):
    s = clip_case(case)
    p, first = s.prog, s.runs[0]
    p.run(first.ids)
    outs = [p.penultimate] + ([p.pooled] if p.pooled is not None else [])
    lifetimes()(p.prog, p.arena, p.prog.launch, lambda: outs)
    assert torch.equal(p.penultimate, first.pen) and (p.pooled is None or torch.equal(p.pooled, first.pooled))


# ---------------------------------------------------------------------------------------------------------------- LPIPS cases
def lpips_frames(case):
    c = LPIPS_CASES[case]
    a, b = TL.smooth_frames(2, c["H"], c["W"], 40 + c["N"])
    if c["N"] == 1:
        return TL.lerp_u8(a, b, 0.3)[None]
    f0 = TL.lerp_u8(a, b, 0.30)                      # neighbours of a transition: lerps at close fractions, and a near-identical frame
    return torch.stack([f0, TL.lerp_u8(a, b, 0.35), TL.lerp_u8(a, b, 0.60), TL.nudge(f0)])


@functools.lru_cache(maxsize=None)
def lpips_net():
    n = native()
    w = R.make_weights(R.lpips_spec(), 7)
    return n.pipe.NativeLPIPS(n.SyntheticProvider(7), DEV), w, MU.evs(w)


@functools.lru_cache(maxsize=None)
def lpips_case(case):
    lp, w, (ref, model) = lpips_net()
    c = LPIPS_CASES[case]
    frames = lpips_frames(case)
    plans = []
    with gemm_census(plans):
        dev_taps = lp.features(frames.to(DEV))
    torch.cuda.synchronize()
    geo = TL.lpips_geometry(c["H"], c["W"])
    taps = {f"conv{i + 1}": TL.tap_nchw(t, geo[i][2], geo[i][3]) for i, t in enumerate(dev_taps)}
    taps["frames"] = frames
    return types.SimpleNamespace(case=case, c=c, lp=lp, w=w, ref=ref, model=model, frames=frames, dev_taps=dev_taps, taps=taps,
                                 plans=plans, geo=geo)


def per_frame(dev_taps, i):
    return [t[i] for t in dev_taps]


def log_census(s, results_log):
    assert [(p["M"], p["N"]) for p in s.plans] == [(s.c["N"] * g[2] * g[3], g[4]) for g in s.geo] and all(p["conv"] for p in s.plans)
    results_log[f"units_lpips_{s.case}/census"] = s.plans
    print(f"[units] lpips {s.case} census: " + " ".join(f"conv{i + 1}:M{p['M']}:r{p['route']}t{p['tile']}k{p['splitk']}" for i, p in enumerate(s.plans)))


def test_lpips_census_leaves_tile_3_and_splits(results_log):
    """Across the cases at least one conv runs on a tile other than 3 and at least one splits along K - the routes of the production
    frame that the 96 x 96 test never reaches."""
    plans = []
    for case in LPIPS_CASES:
        s = lpips_case(case)
        log_census(s, results_log)
        plans += s.plans
    assert any(p["tile"] != 3 for p in plans), plans
    assert any(p["splitk"] > 1 for p in plans), plans
    assert all(p["flags"] & lib().GEMM_RELU for p in plans)


@pytest.mark.parametrize("case,name,src", [pytest.param(case, name, ins[0], id=f"{case}-{name}")
                                           for case in ("batch4_515", "single_259x291") for name, ins in TL.lpips_units()])
def test_lpips_conv_unit_matches_fp64(case, name, src, results_log):
    """Teacher-forced: prep (conv1) or the exact max-pool of the native previous tap, the conv in float64, bias, ReLU."""
    s = lpips_case(case)
    ref64, model = TL.lpips_unit(s.ref, name, s.taps[src]), TL.lpips_unit(s.model, name, s.taps[src])
    bad = MU.compare(results_log, f"units_lpips_{case}/{name}", s.taps[name], model, ref64)
    assert bad is None, bad


@pytest.mark.parametrize("name", ["conv2", "conv4", "conv5"])
def test_lpips_production_frame_units(name, results_log):
    """One 1024^2 frame - the production call itself: conv2 on its large-M tile, conv4 and conv5 split along K under the ReLU
    epilogue.  Features only.  The float64 references of all three (127^2 x 192 x 1600, 63^2 x 256 x 3456, 63^2 x 256 x 2304
    multiply-adds) take a second or two on 16 CPU threads, so none had to be cut down."""
    s = lpips_case("single_1024")
    src = f"conv{int(name[4:]) - 1}"
    t0 = time.time()
    ref64, model = TL.lpips_unit(s.ref, name, s.taps[src]), TL.lpips_unit(s.model, name, s.taps[src])
    print(f"[units] single_1024 {name}: references in {time.time() - t0:.1f} s")
    bad = MU.compare(results_log, f"units_lpips_single_1024/{name}", s.taps[name], model, ref64)
    assert bad is None, bad


def test_lpips_single_frame_against_its_batch_of_two(results_log):
    """N = 1 (odd pooling floors, non-square) and the same frame as the second of a batch of 2: both within the unit bound; whether
    they are the same bits is logged, not asserted (another M may be another tile, another summation order)."""
    s = lpips_case("single_259x291")
    other = TL.smooth_frames(1, s.c["H"], s.c["W"], 77)[0]
    two = s.lp.features(torch.stack([other, s.frames[0]]).to(DEV))
    torch.cuda.synchronize()
    equal, fails = {}, []
    for i, (name, ins) in enumerate(TL.lpips_units()):
        mine = TL.tap_nchw(two[i], s.geo[i][2], s.geo[i][3])[1:2]
        equal[name] = bool(torch.equal(mine, s.taps[name]))
        src = s.taps[ins[0]]                                    # teacher-forced on the N = 1 run's tap
        if name != "conv1":                                      # ... unless the batched run's own input differs from it
            src = TL.tap_nchw(two[i - 1], s.geo[i - 1][2], s.geo[i - 1][3])[1:2]
        ref64, model = TL.lpips_unit(s.ref, name, src), TL.lpips_unit(s.model, name, src)
        fails.append(MU.compare(results_log, f"units_lpips_single_259x291/in_batch_of_2/{name}", mine, model, ref64))
    results_log["units_lpips_single_259x291/bit_equal_in_batch_of_2"] = equal
    print(f"[units] lpips single frame against its batch of 2, bit-equal: {equal}")
    fails = [f for f in fails if f]
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------- LPIPS distances
ORDINARY = [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)]
NEAR = [(0, 3)]


def _all_pairs():
    return [p for a, b in ORDINARY + NEAR for p in ((a, b), (b, a))]


@functools.lru_cache(maxsize=None)
def lpips_distances():
    s = lpips_case("batch4_515")
    pairs = _all_pairs()
    got = s.lp.distances([(per_frame(s.dev_taps, a), per_frame(s.dev_taps, b)) for a, b in pairs]).cpu()
    return pairs, got


def test_lpips_distance_unit(results_log):
    """The distance kernels on the NATIVE fp16 taps against the float64 formula on the same taps.  Every addend of every sum is
    non-negative, so n additions rounded to fp32 stay within n * 2^-24 of the exact sum, relatively; per tap the longest chain of
    additions is L = C / 64 (a lane's channels) + 6 (the wave sum) + ceil(HW / (4 nblk)) (a wave's pixels) + 4 (the block's four
    waves, the accumulator; the sum over blocks is taken in double), and 16 more roundings cover the arithmetic of one element and the
    final scaling: |d - ref| <= sum over taps of (L + 16) * 2^-24 * ref_tap (``lpips_distance_bound``)."""
    s = lpips_case("batch4_515")
    pairs, got = lpips_distances()
    assert got.dtype == F32
    shapes = [(g[2] * g[3], g[4]) for g in s.geo]
    names = TL.LPIPS_TAPS
    log, fails = {}, []
    for (a, b), d in zip(pairs, got.tolist()):
        terms = TL.lpips_tap_terms(s.ref, [s.taps[n][a] for n in names], [s.taps[n][b] for n in names])
        ref, bound = float(terms.sum()), TL.lpips_distance_bound(terms, shapes)
        log[f"{a}-{b}"] = {"native": d, "ref": ref, "error": abs(d - ref), "bound": bound}
        print(f"[units] lpips d({a},{b}): native {d:.9e} ref {ref:.9e} error {abs(d - ref):.2e} bound {bound:.2e}")
        if not (ref > 0 and abs(d - ref) <= bound):
            fails.append((a, b, d, ref, bound))
    results_log["units_lpips_batch4_515/distance_unit"] = log
    assert not fails, fails


def test_lpips_free_running_distances(results_log):
    """All pairs against float64 from the uint8 frames; the yardstick is the free-running storage model.  One scalar's model error can
    vanish by luck, so pairs of similar size are grouped (the ordinary pairs; the near-identical pair and its mirror) and the native
    RMS and max relative errors of a group are held to FACTOR x the model's."""
    s = lpips_case("batch4_515")
    pairs, got = lpips_distances()
    t_ref, t_model = TL.lpips_forward(s.ref, s.frames), TL.lpips_forward(s.model, s.frames)

    def dist(ev, taps, a, b):
        return float(TL.lpips_tap_terms(ev, [t[a] for t in taps], [t[b] for t in taps]).sum())
    groups = {"ordinary": [p for a, b in ORDINARY for p in ((a, b), (b, a))], "near_identical": [p for a, b in NEAR for p in ((a, b), (b, a))]}
    fails = []
    for gname, members in groups.items():
        e_n, e_m = [], []
        for a, b in members:
            ref = dist(s.ref, t_ref, a, b)
            e_n.append((float(got[pairs.index((a, b))]) - ref) / ref)
            e_m.append((dist(s.model, t_model, a, b) - ref) / ref)
        e_n, e_m = torch.tensor(e_n, dtype=F64), torch.tensor(e_m, dtype=F64)
        rec = {"native_rms": float(e_n.pow(2).mean().sqrt()), "model_rms": float(e_m.pow(2).mean().sqrt()),
               "native_max": float(e_n.abs().max()), "model_max": float(e_m.abs().max())}
        results_log[f"units_lpips_batch4_515/free_running/{gname}"] = rec
        print(f"[units] lpips free-running {gname}: " + " ".join(f"{k}={v:.3e}" for k, v in rec.items()))
        if not (rec["native_rms"] <= MU.FACTOR * rec["model_rms"] and rec["native_max"] <= MU.FACTOR * rec["model_max"]):
            fails.append((gname, rec))
    assert not fails, fails


def test_lpips_exact_properties():
    """37 pairs from the 4 frames - three chunks of 16, with repeats: d(a, a) is 0.0; d(a, b) and d(b, a) are the same bits; a repeated
    pair gives the same bits in every slot and chunk; a second call gives the bits of the first (the accumulator is zeroed again)."""
    s = lpips_case("batch4_515")
    f = [per_frame(s.dev_taps, i) for i in range(4)]
    idx = [(a, b) for a in range(4) for b in range(4)]                  # 16: every ordered pair, the diagonal included
    idx = idx + [(0, 1)] + idx[::-1] + [(3, 0), (2, 1), (0, 1), (1, 0)]  # 37: repeats in other slots and other chunks
    assert len(idx) >= 35
    got = s.lp.distances([(f[a], f[b]) for a, b in idx]).cpu()
    again = s.lp.distances([(f[a], f[b]) for a, b in idx]).cpu()
    assert got.dtype == F32 and torch.equal(got, again)
    seen = {}
    for (a, b), d in zip(idx, got.tolist()):
        if a == b:
            assert d == 0.0, (a, b, d)
        else:
            assert d > 0.0
        assert seen.setdefault((a, b), d) == d, f"d({a},{b}) differs between slots: {seen[(a, b)]!r} and {d!r}"
    for (a, b), d in seen.items():
        assert seen[(b, a)] == d, f"d({a},{b}) = {d!r} but d({b},{a}) = {seen[(b, a)]!r}"
    pairs, first = lpips_distances()                                     # ... and the bits of the 12-pair call of the other tests
    assert all(seen[p] == d for p, d in zip(pairs, first.tolist()))
