"""The emitter's path to the K-split form of the 3x3 halo-tile conv (Emitter._halo_ksplit, native/runtime.py: where the K-split
part of lb_conv_plan's record is applied): one workspace per
emitter, shared by every flagged launch; each launch's counters end where the slabs begin; a grown workspace retires the old one,
which recorded ops keep using; the counter area stays zero.  Small 3x3 convs through Emitter.gemm under lb_gemm_set_halo(2) and
lb_conv_halo_set_ksplit(2, 0) - every eligible conv routed to the halo kernel and split, on min(CUs, units) blocks -, held to a
float64 conv of the input each one actually read and, bit for bit, to direct launches of lb_conv3x3_halo_f16.

The 1 MiB cap of the counter area (a launch of more than 262,144 tiles is left unflagged) is not reached here."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _ksplit import DEV, F16, F32, SLAB_BYTES, ksplit_plan, lib, run_conv  # noqa: E402
from _parity import check_close, check_elementwise, contraction_bound, rnd  # noqa: E402

NAN = float("nan")
# (B, H, W, Cin, N, statistics): a chain of three on one (1, 16, 32) image - 8, 24 and 10 units -, then an independent conv of 80 units
CONVS = [(1, 16, 32, 128, 256, False), (1, 16, 32, 256, 320, True), (1, 16, 32, 320, 128, False), (2, 32, 32, 640, 128, False)]


@pytest.fixture(autouse=True)
def switches():
    """Recorded ops read the switches when they are replayed: set for the life of each test."""
    api = lib().api
    api.lb_gemm_set_halo(2)
    api.lb_conv_halo_set_ksplit(2, 0)
    yield api
    api.lb_conv_halo_set_ksplit(1, 0)
    api.lb_gemm_set_halo(1)


@functools.lru_cache(maxsize=None)
def weights():
    """Per conv (w [N, Cin, 3, 3] on the CPU, packed weight on the device, bias fp32 on the CPU, on the device): never modified."""
    from latentblending_amd.hip import ops as o
    out = []
    for i, (_, _, _, cin, n, _) in enumerate(CONVS):
        w, bias = rnd(n, cin, 3, 3, seed=801 + 2 * i, scale=(9 * cin) ** -0.5), rnd(n, seed=802 + 2 * i, dtype=F32)
        out.append((w, o.pack_conv_weight(w, cin).to(DEV), bias, bias.to(DEV)))
    return out


@functools.lru_cache(maxsize=None)
def inputs(scale):
    """(input of the chain, input of the independent conv), NHWC fp16 on the CPU."""
    return rnd(1, 16, 32, 128, seed=811, scale=scale), rnd(2, 32, 32, 640, seed=812, scale=scale)


class Chain:
    """An Arena, an Emitter and the buffers of the four convs: acts[0] -> acts[1] -> acts[2] -> acts[3], big_in -> big_out."""

    def __init__(self, halo_ksplit=True):
        from latentblending_amd.native.runtime import Arena, Emitter
        self.arena = Arena(torch.device(DEV, torch.cuda.current_device()))
        self.em = Emitter(self.arena)
        self.em.halo_ksplit = halo_ksplit
        self.acts = [self.arena.alloc((512, 128))] + [self.arena.alloc((512, c[4])) for c in CONVS[:3]]
        self.big_in, self.big_out = self.arena.alloc((2048, 640)), self.arena.alloc((2048, 128))
        self.rows = self.em.halo_stat_rows(1, 16, 32, 256, 320)
        assert self.rows == 8, "the 256 -> 320 conv must run on the halo kernel: 2 tiles x 4 wave rows"
        self.stats = self.arena.alloc((320, self.rows, 2), F32)
        self.seen = []                                   # per emit: (flagged, a copy of the params, the emitter's workspace then)
        inner = self.em._halo_ksplit

        def spy(p, plan):
            flagged = inner(p, plan)
            self.seen.append((flagged, type(p).from_buffer_copy(p), self.em.ws_ksplit))
            return flagged
        self.em._halo_ksplit = spy

    def fill(self, scale):
        x0, xb = inputs(scale)
        self.acts[0].copy_(x0.reshape(512, 128))
        self.big_in.copy_(xb.reshape(2048, 640))

    def poison(self):
        for t in self.acts[1:] + [self.big_out, self.stats]:
            t.fill_(NAN)

    def io(self, i):
        return (self.acts[i], self.acts[i + 1]) if i < 3 else (self.big_in, self.big_out)

    def emit(self, i):
        B, H, W, cin, n, with_stats = CONVS[i]
        _, wd, _, bd = weights()[i]
        src, dst = self.io(i)
        self.em.gemm(src, wd, dst, M=B * H * W, bias=bd, ch_stats=self.stats if with_stats else None,
                     conv=lib().ConvGeom.conv3x3(H, W, cin))

    def emit_all(self):
        for i in range(len(CONVS)):
            self.emit(i)

    def results(self):
        return [t.clone() for t in self.acts[1:] + [self.big_out, self.stats]]


def _counter_areas_zero(em):
    for buf in [em.ws_ksplit] + [t for t in em._retired if t.dtype == torch.uint8]:
        assert int(buf[:em._KSPLIT_COUNTER_BYTES].max()) == 0, "a launch left a counter of the shared workspace non-zero"


def test_chain_shares_one_workspace_and_grows_it(results_log):
    api = lib().api
    ch = Chain()
    ch.fill(1.0)
    ch.poison()
    ws_after = []
    for i in range(len(CONVS)):
        ch.emit(i)
        ws_after.append(ch.em.ws_ksplit)
    torch.cuda.synchronize()
    em = ch.em
    assert ws_after[0] is not None and ws_after[0].dtype == torch.uint8
    # ---- one workspace, grown: every superseded buffer is kept (recorded ops would still point into it)
    assert ws_after[3] is em.ws_ksplit and ws_after[3] is not ws_after[0] and ws_after[3].numel() > ws_after[0].numel()
    assert ws_after[2] is ws_after[1], "a launch that fits the workspace must not replace it"
    for old in {id(t): t for t in ws_after if t is not em.ws_ksplit}.values():
        assert any(old is t for t in em._retired), "a superseded workspace was dropped"
    # ---- every launch is flagged, and its counters end exactly where the slab area begins (sizes: the plan's own)
    assert [f for f, _, _ in ch.seen] == [True] * 4
    for i, (_, p, ws) in enumerate(ch.seen):
        assert ws is ws_after[i] and p.flags & lib().GEMM_HALO_KSPLIT
        units, grid, split = ksplit_plan(p)
        need = api.lb_conv_halo_ksplit_workspace_bytes(p)
        B, H, W, cin, n, _ = CONVS[i]
        assert split == 1 and units == (B * H * W // 256) * ((n + 127) // 128) * (cin // 64) and grid == units
        counters = need - 2 * grid * SLAB_BYTES
        assert 0 < counters <= em._KSPLIT_COUNTER_BYTES
        assert p.partial + counters == ws.data_ptr() + em._KSPLIT_COUNTER_BYTES
        assert p.partial >= ws.data_ptr() and p.partial + need <= ws.data_ptr() + ws.numel()
    # ---- values: fp64 conv of the input each conv read; bits: a direct flagged launch on a private workspace
    for i, (B, H, W, cin, n, with_stats) in enumerate(CONVS):
        w, wd, bias, bd = weights()[i]
        src, dst = ch.io(i)
        x = src.cpu().reshape(B, H, W, cin)
        x64 = x.double().permute(0, 3, 1, 2)
        ref = F.conv2d(x64, w.double(), padding=1).permute(0, 2, 3, 1) + bias.double()
        ad = F.conv2d(x64.abs(), w.double().abs(), padding=1).permute(0, 2, 3, 1)
        name = f"emk_conv{i}"
        check_elementwise(results_log, name, dst.reshape(B, H, W, n), ref, contraction_bound(None, None, 9 * cin, ref, bias=bias, absdot64=ad))
        st = torch.full((n, B * ch.rows, 2), NAN, dtype=F32, device=DEV) if with_stats else None
        direct = run_conv(src.reshape(B, H, W, cin), wd, bias=bd, stats=st)
        assert torch.equal(dst, direct), f"conv {i}: the emitted launch differs from the direct one"
        if with_stats:
            assert torch.equal(ch.stats, st) and bool(torch.isfinite(st).all()), "every (row block, channel) slot must be written"
            yf = ref.reshape(B, H * W, n)
            tot = ch.stats.reshape(n, B, ch.rows, 2).double().sum(dim=2).permute(1, 0, 2).cpu()
            check_close(results_log, name + "_sum", tot[..., 0], yf.sum(dim=1))
            check_close(results_log, name + "_sumsq", tot[..., 1], (yf ** 2).sum(dim=1))
            stored = dst.double().reshape(B, H * W, n).cpu()          # and tightly: they are the statistics of what was STORED
            assert torch.allclose(tot[..., 0], stored.sum(dim=1), rtol=1e-4, atol=1e-2)
            assert torch.allclose(tot[..., 1], (stored ** 2).sum(dim=1), rtol=1e-4, atol=1e-2)
    _counter_areas_zero(em)


def test_recorded_chain_replays_through_the_retired_workspace():
    """Record the four emits once; replay, instantiate, graph-launch, refill the inputs, graph-launch again: every time the bits of
    an eager emission on the same values - the first convs' recorded ops point into workspaces retired while recording."""
    from latentblending_amd.native.runtime import Program
    eager = Chain()
    want = {}
    for scale in (1.0, 2.5):
        eager.fill(scale)
        eager.poison()
        eager.emit_all()
        want[scale] = eager.results()
    assert not torch.equal(want[1.0][0], want[2.5][0])

    ch = Chain()
    ch.fill(1.0)
    ch.poison()
    prog = Program("emk_chain")
    with prog.record():
        ch.emit_all()
    prog.keep += [ch.arena, ch.em]
    assert prog.op_names() == ["lb_conv3x3_halo_f16"] * 4 and all(bool(torch.isnan(t).all()) for t in ch.results())
    assert ch.seen[0][2] is not ch.em.ws_ksplit and any(ch.seen[0][2] is t for t in ch.em._retired)

    def same(scale, what):
        for i, (got, ref) in enumerate(zip(ch.results(), want[scale])):
            assert torch.equal(got, ref), f"{what}: result {i} differs from the eager emission"
    prog.run()
    same(1.0, "replay")
    prog.instantiate()
    for k in range(2):
        ch.poison()
        prog.launch()
        same(1.0, f"graph launch {k}")
    ch.fill(2.5)
    ch.poison()
    prog.launch()
    same(2.5, "graph launch on new inputs")
    ch.fill(1.0)
    prog.launch()
    same(1.0, "graph launch back on the first inputs")
    torch.cuda.synchronize()
    _counter_areas_zero(ch.em)
    _counter_areas_zero(eager.em)


@pytest.mark.parametrize("how", ["halo_ksplit_false", "mode_0"])
def test_emitter_flags_nothing_when_switched_off(how, switches):
    """Emitter.halo_ksplit = False, or the library's switch at "never": no flag, no workspace, the bits of the unflagged kernel."""
    if how == "mode_0":
        switches.lb_conv_halo_set_ksplit(0, 0)
    ch = Chain(halo_ksplit=how == "mode_0")
    ch.fill(1.0)
    ch.poison()
    ch.emit_all()
    assert ch.em.ws_ksplit is None
    assert [f for f, _, _ in ch.seen] == [False] * 4 and not any(p.flags & lib().GEMM_HALO_KSPLIT for _, p, _ in ch.seen)
    for i, (B, H, W, cin, n, with_stats) in enumerate(CONVS):
        _, wd, _, bd = weights()[i]
        src, dst = ch.io(i)
        st = torch.full((n, B * ch.rows, 2), NAN, dtype=F32, device=DEV) if with_stats else None
        plain = run_conv(src.reshape(B, H, W, cin), wd, split=False, bias=bd, stats=st)
        assert bool(torch.isfinite(plain).all()) and torch.equal(dst, plain), f"conv {i}: differs from the unflagged launch"
        assert not with_stats or torch.equal(ch.stats, st)
