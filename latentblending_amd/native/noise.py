"""Counter-based sampler noise: every value is a pure function of (which trajectory, which step, which element).

This module is the DEFINITION of the stream - ``philox4x32_10`` and ``counter_normal_f16`` restate in numpy float64 what
``lb_counter_noise_f16`` (csrc/noise.hip, contract: include/lb_hip.h) evaluates on the device - and its CPU implementation.

Stream.  Element ``e`` of a draw takes word ``e % 4`` of Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2,
3", SC'11; the Random123 construction) at counter ``{e // 4, ctr1, ctr2, ctr3}`` under key ``{key0, key1}``.  Words become normals in
pairs, (w0, w1) -> elements 0 and 1, (w2, w3) -> elements 2 and 3::

    u1 = ((wa >> 8) + 0.5) 2^-24     t = ((wb >> 8) + 0.5) 2^-23 (= 2 u2)     r = sqrt(-2 ln u1)
    z_even = r cospi(t)              z_odd = r sinpi(t)

in float64, rounded once to fp16.  ``u1 >= 2^-25``, so ``|z| <= sqrt(50 ln 2) < 5.89``.

Rows.  A draw is addressed by a row ``(key0, key1, ctr1, ctr2, ctr3)``: the key is the 64-bit ``trajectory_id`` (low word first),
``ctr1`` the schedule's step index, ``ctr2`` the draw kind (``DRAW_STEP`` = 0: the per-step sampler noise; other values are free
for later kinds of draw), ``ctr3`` = 0.

Identities.  ``trajectory_id(tag, *words)`` folds its 64-bit words with SplitMix64's finaliser (Steele, Lea, Flood 2014)::

    h = 0;  for w in (tag, *words):  h = mix64((h + 0x9E3779B97F4A7C15 + w) mod 2^64)
    mix64(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31

* an anchor is ``(TAG_ANCHOR, seed)`` - the same seed is the same trajectory as anchor 1, anchor 2 or a precomputed key frame;
* a mid branch is ``(TAG_MID, seed1, seed2, float64 bits of fract_mixing, idx_injection)``;
* a caller that binds nothing is ``(TAG_FREE, source seed, running call count)``.

What stays stream-based: the START latent of a trajectory (``get_noise(seed)``: a host generator seeded with the seed, as the
reference draws it) and everything under ``noise="stream"``.
"""
from __future__ import annotations

import struct
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

TAG_ANCHOR, TAG_MID, TAG_FREE = 1, 2, 3
DRAW_STEP = 0                         # ctr2: the per-step sampler noise (ancestral / LCM re-noising)

_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def _mix64(z: int) -> int:
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def trajectory_id(tag: int, *words: int) -> int:
    """The 64-bit identity of a trajectory: ``(tag, *words)`` (each taken mod 2^64) folded as the module text states."""
    h = 0
    for w in (tag,) + tuple(words):
        h = _mix64(h + _GOLDEN + (int(w) & _M64))
    return h


def anchor_id(seed: int) -> int:
    return trajectory_id(TAG_ANCHOR, int(seed))


def mid_id(seed1: int, seed2: int, fract_mixing: float, idx_injection: int) -> int:
    bits = struct.unpack("<Q", struct.pack("<d", float(fract_mixing)))[0]
    return trajectory_id(TAG_MID, int(seed1), int(seed2), bits, int(idx_injection))


def free_id(seed: int, count: int) -> int:
    return trajectory_id(TAG_FREE, int(seed), int(count))


def noise_row(tid: int, step: int, kind: int = DRAW_STEP) -> Tuple[int, int, int, int, int]:
    """``(key0, key1, ctr1, ctr2, ctr3)`` of the draw of kind ``kind`` that trajectory ``tid`` makes at schedule step ``step``."""
    tid = int(tid) & _M64
    return (tid & 0xFFFFFFFF, tid >> 32, int(step) & 0xFFFFFFFF, int(kind) & 0xFFFFFFFF, 0)


def philox4x32_10(ctr, key) -> np.ndarray:
    """Philox4x32-10 over arrays: ``ctr`` [..., 4] and ``key`` [..., 2] of 32-bit words (broadcast against each other) ->
    uint32 [..., 4]."""
    ctr = np.asarray(ctr, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    key = np.asarray(key, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(ctr[..., k], shape).copy() for k in range(4)]
    k0, k1 = np.broadcast_to(key[..., 0], shape).copy(), np.broadcast_to(key[..., 1], shape).copy()
    lo = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c[0], np.uint64(PHILOX_M1) * c[2]          # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & lo, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & lo]
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & lo, (k1 + np.uint64(PHILOX_W1)) & lo
    return np.stack(c, axis=-1).astype(np.uint32)


def counter_words(rows: Sequence[Sequence[int]], per_sample: int) -> np.ndarray:
    """uint32 [n, per_sample]: the Philox words of ``rows`` (what the launcher stores with ``raw = 1``)."""
    n, per_sample = len(rows), int(per_sample)
    if per_sample <= 0 or per_sample % 4:
        raise ValueError(f"counter_words: per_sample must be a positive multiple of 4 (got {per_sample})")
    r = np.asarray([[int(v) & 0xFFFFFFFF for v in row] for row in rows], dtype=np.uint64).reshape(n, 5)
    ctr = np.zeros((n, per_sample // 4, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(per_sample // 4, dtype=np.uint64)[None, :]
    ctr[..., 1:] = r[:, None, 2:5]
    return philox4x32_10(ctr, r[:, None, 0:2]).reshape(n, per_sample)


def _sincospi(t: np.ndarray):
    """(sinpi(t), cospi(t)) in float64 for ``t`` in [0, 2]: the argument is reduced EXACTLY (t is a dyadic rational) to
    r = t - q / 2 in [-1/4, 1/4] before pi enters, so the zeros of both functions keep their relative accuracy."""
    q = np.rint(2.0 * t)
    r = t - 0.5 * q
    s, c = np.sin(np.pi * r), np.cos(np.pi * r)
    q = q.astype(np.int64) & 3
    sn = np.choose(q, [s, c, -s, -c])
    cs = np.choose(q, [c, -s, -c, s])
    return sn, cs


def normals_from_words(w: np.ndarray) -> np.ndarray:
    """uint32 [n, per_sample] words -> float64 [n, per_sample] normals: the transform alone."""
    w = np.asarray(w, dtype=np.uint32)
    wa, wb = w[:, 0::2], w[:, 1::2]
    u1 = ((wa >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    t = ((wb >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -23
    r = np.sqrt(-2.0 * np.log(u1))
    sn, cs = _sincospi(t)
    z = np.empty(w.shape, dtype=np.float64)
    z[:, 0::2] = r * cs
    z[:, 1::2] = r * sn
    return z


def counter_normal_f64(rows: Sequence[Sequence[int]], per_sample: int) -> np.ndarray:
    """float64 [n, per_sample]: the normals before the one rounding to fp16."""
    return normals_from_words(counter_words(rows, per_sample))


def counter_normal_f16(rows: Sequence[Sequence[int]], per_sample: int) -> np.ndarray:
    """float16 [n, per_sample]: the stream ``lb_counter_noise_f16`` produces for ``rows`` (the CPU implementation)."""
    if int(per_sample) <= 0 or int(per_sample) % 8:
        raise ValueError(f"counter_normal_f16: per_sample must be a positive multiple of 8 (got {per_sample})")
    return counter_normal_f64(rows, per_sample).astype(np.float16)


class CounterNoise:
    """Noise source for ``scheduler.noise_source`` whose draws are addressed, not consumed.

    ``keyed(ids_and_steps, shape)`` is what the native loops call: ``ids_and_steps`` = [(trajectory id, step), ...], ``shape`` =
    (n, ...) -> fp16 of that shape on the source's device; ONE ``ops.counter_noise`` launch on a GPU device, the numpy
    restatement on ``cpu``.  ``bind(ids)`` + ``__call__(shape)`` serve the generic ``scheduler.step()`` path: a draw takes the
    bound id(s) - one id, or one per sample of the batch - and the step index of ``scheduler`` (the attribute; the owner of the
    source sets it).  Unbound calls and ``many`` exist so that foreign code keeps working: they take ``TAG_FREE`` ids from the
    source's seed and its running call count - a stream again, and documented as such."""

    def __init__(self, device="cuda", seed: int = 0, scheduler=None):
        self.device = torch.device(device)
        self.seed = int(seed)
        self.scheduler = scheduler
        self._bound = None
        self._free_calls = 0

    # ---- addressed draws ----------------------------------------------------------------------
    def keyed(self, ids_and_steps, shape) -> torch.Tensor:
        shape = tuple(int(s) for s in shape)
        rows = [noise_row(tid, step) for tid, step in ids_and_steps]
        if len(rows) != shape[0]:
            raise ValueError(f"CounterNoise.keyed: {len(rows)} (id, step) pairs for a draw of shape {shape}")
        if not rows:
            return torch.empty(shape, dtype=torch.float16, device=self.device)
        if self.device.type == "cpu":
            per_sample = int(np.prod(shape[1:]))
            return torch.from_numpy(counter_normal_f16(rows, per_sample)).reshape(shape)
        from ..hip import ops
        return ops.counter_noise(rows, shape, device=self.device)

    # ---- the generic step() path --------------------------------------------------------------
    def bind(self, ids) -> Optional[object]:
        """Bind the id (or one id per sample) of the trajectory the next ``__call__`` draws belong to; ``None`` unbinds.
        Returns what was bound before."""
        before, self._bound = self._bound, ids
        return before

    def bound_id(self) -> int:
        """The id a single-sample run draws under: the bound one, else the next ``TAG_FREE`` id."""
        if self._bound is not None:
            return int(self._bound) if isinstance(self._bound, int) else int(list(self._bound)[0])
        self._free_calls += 1
        return free_id(self.seed, self._free_calls - 1)

    def _step_index(self) -> int:
        i = getattr(self.scheduler, "_step_index", None)
        if i is None:
            raise RuntimeError("CounterNoise: a bound draw needs `scheduler` (the object whose step() draws) with a located step")
        return int(i)

    def __call__(self, shape) -> torch.Tensor:
        shape = tuple(int(s) for s in shape)
        if self._bound is None:
            return self.many(shape[0], shape)
        ids = [self._bound] * shape[0] if isinstance(self._bound, int) else list(self._bound)
        step = self._step_index()
        return self.keyed([(t, step) for t in ids], shape)

    def many(self, n: int, shape) -> torch.Tensor:
        """``n`` unbound draws of ``shape[1:]``: ``TAG_FREE`` ids, one per draw, step 0."""
        n = int(n)
        ids = [(free_id(self.seed, self._free_calls + k), 0) for k in range(n)]
        self._free_calls += n
        return self.keyed(ids, (n,) + tuple(shape[1:]))
