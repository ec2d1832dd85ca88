"""Seeded inputs and the parity checks shared by the per-kernel GPU tests (test_kernels_gpu.py, test_kernel_bounds_gpu.py)."""
import torch


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def ulp_diff_f16(a, b):
    ai = a.cpu().view(torch.int16).to(torch.int32)
    bi = b.cpu().view(torch.int16).to(torch.int32)
    ai = torch.where(ai < 0, -32768 - ai, ai)
    bi = torch.where(bi < 0, -32768 - bi, bi)
    return int((ai - bi).abs().max())


def check_close(log, name, got, ref, rel=2e-3, frac=2 ** -8, floor=1e-3):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    err = (got - ref).abs().max().item()
    rl2 = ((got - ref).norm() / (ref.norm() + 1e-30)).item()
    bound = frac * ref.abs().max().item() + floor
    log[name] = {"max_abs": err, "rel_l2": rl2, "bound_abs": bound}
    print(f"[parity] {name}: max_abs={err:.3e} (bound {bound:.3e}) rel_l2={rl2:.3e}")
    assert rl2 <= rel, f"{name}: rel-L2 {rl2:.3e} > {rel}"
    assert err <= bound, f"{name}: max-abs {err:.3e} > {bound:.3e}"
