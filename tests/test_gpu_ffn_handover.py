"""The hidden-chunk hand-over of the row-panel FFN kernels (csrc/ffn_x6.hip: egtr_ffn_x6_f32, egtr_encoder_tail_x6_f32).

Layer 1 runs one hidden chunk (64 units) ahead of layer 2, and the chunk in between is handed over -- bias, ReLU, split,
twelve LDS stores per lane -- behind layer 2's matrix instructions of the chunk before.  What can go wrong with that order is a
chunk read stale, read twice, skipped, or multiplied with another chunk's layer-2 weights; the shapes are the smallest that
reach every case of the walk: 1, 2, 3 and 4 chunks (F = 64 .. 256: no, one, two and three steady-state rounds), partial last
panels, and several workgroups so that the rotated chunk order (workgroup b starts at chunk b mod nchunk) wraps:
130 rows at F = 128 are three workgroups with rotations 0, 1, 0; 200 rows at F = 192 four with rotations 0, 1, 2, 0.
"""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(1, 64), (64, 64), (65, 128), (130, 128), (200, 192), (257, 256)]
BAD_ROWS = {63: float("inf"), 64: float("nan")}   # either side of a panel edge


def _modules(F, seed):
    """(out_proj, ln1, fc1, fc2, ln2) with seeded random parameters of the model's magnitudes, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    proj, ln1 = torch.nn.Linear(256, 256), torch.nn.LayerNorm(256)
    fc1, fc2, ln2 = torch.nn.Linear(256, F), torch.nn.Linear(F, 256), torch.nn.LayerNorm(256)
    with torch.no_grad():
        proj.weight.copy_(torch.randn(256, 256, generator=g) / 16)
        proj.bias.copy_(torch.randn(256, generator=g) * 0.3)
        fc1.weight.copy_(torch.randn(F, 256, generator=g) / 16)
        fc1.bias.copy_(torch.randn(F, generator=g) * 0.3)
        fc2.weight.copy_(torch.randn(256, F, generator=g) / F ** 0.5)
        fc2.bias.copy_(torch.randn(256, generator=g) * 0.3)
        for ln in (ln1, ln2):
            ln.weight.copy_(1 + 0.2 * torch.randn(256, generator=g))
            ln.bias.copy_(0.2 * torch.randn(256, generator=g))
    return proj, ln1, fc1, fc2, ln2


def _ffn_ref64(x, fc1, fc2, ln=None):
    x = x.double()
    h = torch.relu(x @ fc1.weight.double().t() + fc1.bias.double())
    y = h @ fc2.weight.double().t() + fc2.bias.double()
    if ln is None:
        return y
    return torch.nn.functional.layer_norm(x + y, (256,), ln.weight.double(), ln.bias.double(), ln.eps)


@functools.lru_cache(maxsize=None)
def operands(M, F):
    """Seeded random operands of one shape: the CPU modules, x = the FFN's input = the tail's context, hid, pos."""
    g = torch.Generator().manual_seed(9000 + 7 * M + F)
    x, hid, pos = (torch.randn(M, 256, generator=g) for _ in range(3))
    return _modules(F, 31 + F), x, hid, pos


def run_kernels(M, F, x=None):
    """Every route through the two entries on the operands of (M, F) (x: another FFN input / tail context):
    FFN without LayerNorm, with it, with it and the position output; the encoder tail without and with the position output."""
    from egtr_amd import ops
    mods, x0, hid, pos = operands(M, F)
    xd = (x0 if x is None else x).to(DEV)
    proj, ln1, fc1, fc2, ln2 = (copy.deepcopy(m).to(DEV) for m in mods)
    with torch.no_grad():
        out = {"ffn_plain": ops.ffn_fused(xd, fc1, fc2), "ffn_ln": ops.ffn_fused(xd, fc1, fc2, ln2)}
        out["ffn_ln_p"], out["ffn_pos"] = ops.ffn_fused(xd, fc1, fc2, ln2, pos.to(DEV))
        out["tail"] = ops.encoder_tail_fused(xd, hid.to(DEV), proj, ln1, fc1, fc2, ln2)
        out["tail_p"], out["tail_pos"] = ops.encoder_tail_fused(xd, hid.to(DEV), proj, ln1, fc1, fc2, ln2, pos.to(DEV))
    return {k: v.cpu() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def clean_run(M, F):
    return run_kernels(M, F)


@pytest.mark.parametrize("M,F", SHAPES)
def test_chunk_markers_exact(M, F):
    """Layer 1 = its bias alone, 1 + c on the units of chunk c; layer 2 sums chunk c into output column c: y[:, c] =
    64 (1 + c), every other column 0 -- small integers, exact in every piece of the split, so the comparison is exact.  A
    chunk handed over stale, twice, not at all, or against another chunk's layer-2 weights is a wrong integer in a known
    column."""
    from egtr_amd import ops
    nchunk = F // 64
    fc1, fc2 = torch.nn.Linear(256, F), torch.nn.Linear(F, 256)
    chunk = torch.arange(F) // 64
    with torch.no_grad():
        fc1.weight.zero_()
        fc1.bias.copy_((1 + chunk).float())
        fc2.weight.copy_((torch.arange(256)[:, None] == chunk[None, :]).float())
        fc2.bias.zero_()
    x = operands(M, F)[1]
    want = torch.zeros(M, 256)
    want[:, :nchunk] = 64.0 * (1 + torch.arange(nchunk)).float()
    assert torch.equal(_ffn_ref64(x, fc1, fc2), want.double())   # the table itself, in float64 on the CPU
    with torch.no_grad():
        y = ops.ffn_fused(x.to(DEV), fc1.to(DEV), fc2.to(DEV)).cpu()
    assert torch.equal(y, want), (y[0, :nchunk + 1].tolist(), (y != want).nonzero()[:4].tolist())


@pytest.mark.parametrize("M,F", SHAPES)
@torch.no_grad()
def test_vs_float64(M, F):
    """Per row no further from float64 than 2.5x the fp32 composition the kernels replace, plus 2e-6 of the row scale (the
    criterion of tests/test_gpu_pinning.py::test_fused_ffn_vs_float64 / ::test_fused_encoder_tail_vs_float64)."""
    (proj, ln1, fc1, fc2, ln2), x, hid, _ = operands(M, F)
    got = clean_run(M, F)
    pd, l1d, f1d, f2d, l2d = (copy.deepcopy(m).to(DEV) for m in (proj, ln1, fc1, fc2, ln2))
    with torch.no_grad():
        xd = x.to(DEV)
        c_plain = f2d(torch.relu(f1d(xd)))
        c_ln = l2d(xd + c_plain)
        y1c = l1d(hid.to(DEV) + pd(xd))
        c_tail = l2d(y1c + f2d(torch.relu(f1d(y1c))))
    y1 = torch.nn.functional.layer_norm(hid.double() + x.double() @ proj.weight.double().t() + proj.bias.double(), (256,),
                                        ln1.weight.double(), ln1.bias.double(), ln1.eps)
    for name, comp, ref in (("ffn_plain", c_plain, _ffn_ref64(x, fc1, fc2)), ("ffn_ln", c_ln, _ffn_ref64(x, fc1, fc2, ln2)),
                            ("tail", c_tail, _ffn_ref64(y1, fc1, fc2, ln2))):
        y = got[name]
        assert torch.isfinite(y).all(), name
        e, e32 = (y.double() - ref).abs(), (comp.cpu().double() - ref).abs()
        scale = ref.abs().amax(1, keepdim=True).clamp_min(1e-30)
        worst, worst32 = (e / scale).amax(1), (e32 / scale).amax(1)
        print(f"{name} M={M} F={F}: kernel {float(worst.max()):.3e}, fp32 composition {float(worst32.max()):.3e} of the row scale")
        assert (worst <= 2.5 * worst32 + 2e-6).all(), (name, float(worst.max()))


@pytest.mark.parametrize("M,F", SHAPES)
def test_reproducible_with_and_without_pos(M, F):
    """A second call gives the same bits, and the position output changes nothing else: y the same bits with and without
    it, y + pos exactly that sum."""
    first, again, pos = clean_run(M, F), run_kernels(M, F), operands(M, F)[3]
    for name in first:
        assert torch.equal(first[name], again[name]), name
    assert torch.equal(first["ffn_ln"], first["ffn_ln_p"]) and torch.equal(first["tail"], first["tail_p"])
    assert torch.equal(first["ffn_pos"], first["ffn_ln"] + pos) and torch.equal(first["tail_pos"], first["tail"] + pos)


@pytest.mark.parametrize("M,F", SHAPES)
def test_non_finite_rows_only(M, F):
    """An inf in row 63 and a NaN in row 64 (the last row of one panel, the first of the next; the rows the shape has) make
    exactly those output rows non-finite; every other row keeps its bits."""
    clean, x = clean_run(M, F), operands(M, F)[1].clone()
    bad = torch.zeros(M, dtype=torch.bool)
    for r, v in BAD_ROWS.items():
        if r < M:
            x[r, (5 * r) % 256] = v
            bad[r] = True
    dirty = run_kernels(M, F, x)
    for name in clean:
        assert torch.equal(clean[name][~bad], dirty[name][~bad]), name
        assert not torch.isfinite(dirty[name][bad]).all(-1).any(), name
