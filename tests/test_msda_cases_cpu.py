"""CPU: the float64 MSDA restatement (tests/msda_restated.py) against the oracle and torch autograd, and the constructed cases
of tests/test_gpu_msda_windows.py against what they are named for."""
import functools

import numpy as np
import pytest
import torch

import msda_restated as R
import weights as W
from oracle import msda as OM

SMALL = [  # (B, Lq, M, D, shapes, P): the small shapes of test_msda_vs_oracle / test_msda_generic_shapes
    (4, 7, 8, 32, [(5, 5), (3, 3), (2, 2), (1, 1)], 4),
    (3, 33, 8, 32, [(8, 8), (4, 4)], 8),
    (1, 200, 8, 32, [(19, 32), (10, 16), (5, 8), (3, 4)], 4),
    (2, 13, 3, 20, [(6, 5), (2, 3)], 2),
    (2, 13, 4, 16, [(7, 9)], 3),
]


@functools.lru_cache(maxsize=None)
def case(name):
    return (R.CASES.get(name) or R.BIG_CASES.get(name) or R.BOUNDARY_CASE)()


def _pyramid(x):
    return [tuple(s) for s in x["shapes"].tolist()]


@pytest.mark.parametrize("B,Lq,M,D,shapes,P", SMALL)
def test_restatement_equals_the_oracle_in_float64(B, Lq, M, D, shapes, P):
    x = W.make_msda_inputs(300 + Lq, B, Lq, M, D, shapes, P, dtype=torch.float64, oob_frac=0.15)
    r = R.msda_backward_budget(x["value"], shapes, x["lsi"].tolist(), x["loc"], x["attn"], x["grad_out"])
    gv, gl, ga = OM.msda_backward(x["value"], x["shapes"], x["lsi"], x["loc"], x["attn"], x["grad_out"])
    for got, want in ((r["grad_value"], gv), (r["grad_loc"], gl), (r["grad_attn"], ga)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    f = R.msda_forward_budget(x["value"], shapes, x["lsi"].tolist(), x["loc"], x["attn"])
    assert float((f["out"] - OM.msda_forward(x["value"], x["shapes"], x["lsi"], x["loc"], x["attn"])).abs().max()) <= 1e-12
    # the budgets dominate their sums, and an element without a term is zero
    for n in ("grad_value", "grad_loc", "grad_attn"):
        assert bool((r[n].abs() <= r["abs_" + n] * (1 + 1e-12)).all())
    assert bool((f["out"].abs() <= f["abs_out"] * (1 + 1e-12)).all())
    assert bool(((r["n_terms"] == 0) == (r["abs_grad_value"] == 0)).all())
    assert int(r["n_terms"].max()) <= Lq * len(shapes) * P


@pytest.mark.parametrize("B,Lq,M,D,shapes,P", SMALL)
def test_restatement_equals_autograd_through_grid_sample(B, Lq, M, D, shapes, P):
    x = W.make_msda_inputs(400 + Lq, B, Lq, M, D, shapes, P, dtype=torch.float64, oob_frac=0.15)
    value, loc, attn = (x[n].clone().requires_grad_(True) for n in ("value", "loc", "attn"))
    out = OM.msda_forward_grid_sample(value, x["shapes"], loc, attn)
    out.backward(x["grad_out"])
    r = R.msda_backward_budget(x["value"], shapes, x["lsi"].tolist(), x["loc"], x["attn"], x["grad_out"])
    f = R.msda_forward_budget(x["value"], shapes, x["lsi"].tolist(), x["loc"], x["attn"])
    assert float((f["out"] - out.detach()).abs().max()) <= 1e-10
    for got, want in ((r["grad_value"], value.grad), (r["grad_loc"], loc.grad), (r["grad_attn"], attn.grad)):
        assert float((got - want).abs().max()) <= 1e-10 * max(1.0, float(want.abs().max()))


def test_quantize_loc():
    loc = torch.rand(1000, dtype=torch.float32) * 3 - 1
    q = R.quantize_loc(loc)
    assert q.dtype == torch.float32 and float((q - loc).abs().max()) <= 2.0 ** -13
    assert bool(((q.double() * R.GRID) == (q.double() * R.GRID).round()).all())
    with pytest.raises(AssertionError):   # an off-grid coordinate is refused
        R.assert_exact_geometry([(8, 8)], torch.full((1, 1, 8, 1, 16, 2), 0.3))


@pytest.mark.parametrize("name", list(R.CASES) + list(R.BIG_CASES) + ["boundary"])
def test_case_geometry_is_exact_and_operands_are_on_their_grids(name):
    x = case(name)
    R.assert_exact_geometry(_pyramid(x), x["loc"])
    a, g = x["attn"].double() * 256, x["grad_out"].double() * 64
    assert bool((a == a.round()).all()) and 0 <= float(a.min()) and float(a.max()) <= 32
    assert bool((g == g.round()).all()) and float(g.abs().max()) <= 256
    assert bool((x["grad_out"].to(torch.bfloat16).float() == x["grad_out"]).all())   # bf16 keeps grad_out exactly
    # about 10 % of the samples out of range, some in the border strip (-1, 0)
    out, strip, n = 0, 0, 0
    for l, (H, Wd) in enumerate(_pyramid(x)):
        px = x["loc"][:, :, :, l, :, 0].double() * Wd - 0.5
        py = x["loc"][:, :, :, l, :, 1].double() * H - 0.5
        valid = (py > -1) & (px > -1) & (py < H) & (px < Wd)
        out += int((~valid).sum())
        strip += int((valid & ((px < 0) | (py < 0))).sum())
        n += valid.numel()
    if name in R.CASES:
        assert 0.05 < out / n < 0.2
    assert strip > 0


@functools.lru_cache(maxsize=None)
def budget(name):
    x = case(name)
    return R.msda_backward_budget(x["value"], _pyramid(x), x["lsi"].tolist(), x["loc"], x["attn"], x["grad_out"])


@pytest.mark.parametrize("name", ["seams", "degenerate", "l1_tile", "gapped"])
def test_fp32_evaluation_meets_the_criteria_and_a_lost_sample_does_not(name):
    """The criteria of the GPU tests are attainable -- the oracle evaluated in fp32 on the CPU (sequential additions) meets
    them -- and sharp: with the contributions of ONE sample of one query removed, grad_value misses them."""
    x, ref = case(name), budget(name)
    args = [x[n] for n in ("value", "shapes", "lsi", "loc", "attn", "grad_out")]
    got = OM.msda_backward(*args)
    R.check_backward(name + " fp32 oracle", got, ref)
    f = R.msda_forward_budget(x["value"], _pyramid(x), x["lsi"].tolist(), x["loc"], x["attn"])
    R.check_forward(name + " fp32 oracle", OM.msda_forward(*args[:5]), f)
    # the valid sample with the smallest nonzero attention x |grad_out| mass of image 0
    B, Lq, Mh, L, P, _ = x["loc"].shape
    mass = x["attn"][0].double() * x["grad_out"][0].double().reshape(Lq, Mh, 1, 1, R.D).abs().sum(-1)   # [Lq, M, L, P]
    for l, (H, Wd) in enumerate(_pyramid(x)):
        px = x["loc"][0, :, :, l, :, 0].double() * Wd - 0.5
        py = x["loc"][0, :, :, l, :, 1].double() * H - 0.5
        mass[:, :, l][~((py > -1) & (px > -1) & (py < H) & (px < Wd))] = 0
    mass[mass == 0] = float("inf")
    q, m, l, p = np.unravel_index(int(mass.argmin()), mass.shape)
    attn = x["attn"].clone()
    attn[0, q, m, l, p] = 0
    lost = OM.msda_backward(args[0], args[1], args[2], args[3], attn, args[5])
    with pytest.raises(AssertionError):
        R.check_backward(name + " one sample lost", (lost[0], got[1], got[2]), ref)


def test_seam_windows_are_what_the_case_is_named_for():
    x = case("seams")
    w = R.tile_windows(_pyramid(x), x["lsi"].tolist(), x["loc"], x["loc"].shape[1])
    assert w["tiles"].shape == (43, 64) and w["ntot"].shape == (R.SEAM_B, 43, 8)
    assert sorted(set(x["expect"].values())) == [1, 31, 32, 33, 447, 448, 449, 895, 896, 897, 2720]
    for (b, tile, head), ntot in x["expect"].items():
        assert int(w["ntot"][b, tile, head]) == ntot, (b, tile, head)
        for l, rect in R.SEAM_WINDOWS[ntot].items():
            assert tuple(w["rect"][b, tile, head, l]) == rect
    # every head: its first target on item `head`, its second on item 32 + head = the first two items of workgroup `head`
    ntiles = w["tiles"].shape[0]
    for head in range(8):
        for j, target in ((head, R.SEAM_FIRST[head]), (R.NPX + head, R.SEAM_SECOND[head])):
            b, tile = R.item_at(j, R.SEAM_B, ntiles)
            assert R.item_of(b, tile, R.SEAM_B, ntiles) == j and x["expect"][(b, tile, head)] == target
    assert R.SEAM_B * ntiles > 2 * R.NPX   # items are left for the counter
    # a level that starts inside a 32-column tile and inside a chunk, and a row width that does not divide the chunk
    for ntot in (447, 448, 449, 895, 896, 897):
        r0 = R.SEAM_WINDOWS[ntot][0]
        vb1, width = (r0[1] - r0[0] + 1) * (r0[3] - r0[2] + 1), r0[3] - r0[2] + 1
        assert vb1 % 32 != 0 and vb1 % 448 != 0 and 448 % width != 0


def test_empty_windows_are_empty():
    x = case("empty")
    w = R.tile_windows(_pyramid(x), x["lsi"].tolist(), x["loc"], x["loc"].shape[1])
    b0, t0 = x["empty_level0"]
    assert bool((w["rect"][b0, t0, :, 0, 1] < w["rect"][b0, t0, :, 0, 0]).all()) and bool((w["ntot"][b0, t0] > 0).all())
    for (b, tile, head), ntot in x["expect"].items():
        assert ntot == 0 and int(w["ntot"][b, tile, head]) == 0
        others = [h for h in range(8) if h != head]
        assert bool((w["ntot"][b, tile, others] > 0).all())
    assert int((w["ntot"] == 0).sum()) == len(x["expect"])


def test_tile_maps():
    # encoder mode: levels tiled in 8 x 8 blocks; degenerate levels give one-row / one-column tiles
    tq = R.tile_queries(R.DEGENERATE_PYRAMID, R.level_starts(R.DEGENERATE_PYRAMID), 291)
    assert tq.shape[0] == 6 + 2 + 2 + 1
    assert sorted(tq[tq >= 0].tolist()) == list(range(291))
    assert tq[6][:9].tolist() == [272, 273, 274, 275, 276, 277, 278, 279, -1] and tq[10].tolist() == [290] + [-1] * 63
    # gapped levels: consecutive queries
    x = case("gapped")
    assert x["value"].shape[1] == 325 and x["loc"].shape[1] == 325
    tq = R.tile_queries(_pyramid(x), x["lsi"].tolist(), 325)
    assert tq.shape[0] == 6 and tq[5][:6].tolist() == [320, 321, 322, 323, 324, -1]
    # the gap rows receive nothing
    r = R.msda_backward_budget(x["value"], _pyramid(x), x["lsi"].tolist(), x["loc"], x["attn"], x["grad_out"])
    assert float(r["abs_grad_value"][:, 256:261].max()) == 0 and float(r["abs_grad_value"][:, 261:].min()) > 0


@pytest.mark.parametrize("name", list(R.BIG_CASES) + ["boundary"])
def test_big_windows_span_every_level(name):
    x = case(name)
    shapes = _pyramid(x)
    S = sum(h * w for h, w in shapes)
    assert (S == 65536 if name == "boundary" else S > 65536) and all(h * w <= 65536 for h, w in shapes[1:]) and x["loc"].shape[1] == S
    w = R.tile_windows(shapes, x["lsi"].tolist(), x["loc"], S)
    ntiles = w["tiles"].shape[0]
    assert x["chosen_tiles"] == [0, ntiles // 2, ntiles - 1]
    for t in x["chosen_tiles"]:
        assert bool((w["ntot"][0, t] == S).all())
        for l, (H, Wd) in enumerate(shapes):
            assert bool((w["rect"][0, t, :, l] == np.array([0, H - 1, 0, Wd - 1])).all())
    rows = x["rows"]
    assert sorted(rows.tolist()) == sorted(q for t in x["chosen_tiles"] for q in w["tiles"][t] if q >= 0)
    keep = torch.zeros(S, dtype=torch.bool)
    keep[rows] = True
    assert float(x["grad_out"][0, ~keep].abs().max()) == 0 and float(x["grad_out"][0, keep].abs().max()) > 0
