"""CPU: the cases of tests/test_gpu_msda_forward_edges.py are what they are named for, the float64 restatement of the fused forward
(tests/msda_forward_restated.py) agrees with the oracle, and the criteria reject a forward with one piece wrong."""
import numpy as np
import pytest
import torch

import msda_forward_restated as FR
import msda_restated as R
from oracle import msda as OM

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
EXACT = list(FR.EXACT_CASES) + list(FR.BITS_CASES)
ODD = list(FR.ODD_FUSED_CASES)


def _selected(x):
    return (x["logit"] == 0).reshape(x["off"].shape[:-1])


@pytest.mark.parametrize("name", EXACT)
def test_exact_cases_meet_the_preconditions(name):
    FR.assert_exact_forward(FR.case(name))


@pytest.mark.parametrize("name", list(FR.EXACT_CASES))
def test_restatement_equals_the_oracle_on_the_exact_cases(name):
    x = FR.case(name)
    for form in ("point", "box"):
        loc, attn = FR.sane(FR.locations(x, form)), FR.attention(x)
        r = FR.reference(x, form)
        assert torch.equal(r["out"], OM.msda_forward(x["value"].double(), x["shapes"], x["lsi"], loc, attn))
        assert torch.equal(r["out"], FR.accumulate(x["value"], x["pyramid"], x["lsi"].tolist(), loc, attn)["out"])
        # the pure-PyTorch fallback of the model source in fp32: grid_sample forms 2 loc - 1 and maps it back, 16 n terms
        gs = OM.msda_forward_grid_sample(x["value"], x["shapes"], loc.float(), attn.float())
        assert float((gs.double() - r["out"]).abs().max()) <= 2.0 ** -16 * max(1.0, float(r["abs_out"].max()))
    # masked with bias: the model source zeroes the padded rows of value_proj(x) + bias
    r = FR.reference(x, "point", mask=True, bias=True)
    v = (x["value"].double() + x["vbias"].double().view(1, 1, FR.M, FR.D)) * x["keep"].double()[:, :, None, None]
    want = OM.msda_forward(v, x["shapes"], x["lsi"], FR.sane(FR.locations(x, "point")), FR.attention(x))
    assert torch.equal(r["out"], want)


def test_slots_hits_every_head_and_slot():
    for name in ("slots", "slots_wave"):
        sel = _selected(FR.case(name)).flatten(3)
        assert bool(sel.flatten(0, 1).any(0).all()) and bool((sel.sum(-1) == 1).all())
    # ... and every (head, slot) carries an output alone that is not zero
    x = FR.case("slots")
    r = FR.reference(x, "point")
    hit = (r["abs_out"].reshape(3 * 37, FR.M, FR.D).sum(-1) > 0)[:, :, None] & _selected(x).flatten(3).flatten(0, 1)
    assert bool(hit.any(0).all())


def test_falloff_contains_every_corner_pattern_on_every_level():
    x = FR.case("falloff")
    loc, sel = FR.locations(x, "point"), _selected(x)
    for l, (H, W) in enumerate(FR.P2):
        s = sel[:, :, :, l]
        px, py = (loc[:, :, :, l, :, 0] * W - 0.5)[s], (loc[:, :, :, l, :, 1] * H - 0.5)[s]
        cls = lambda p, n: torch.where(p.floor() == -1, 0, torch.where(p.floor() == n - 1, 2, 1))  # noqa: E731
        inr = (px > -1) & (px < W) & (py > -1) & (py < H)
        seen = {(int(a), int(b)) for a, b in zip(cls(px, W)[inr], cls(py, H)[inr])}
        assert seen == {(a, b) for a in range(3) for b in range(3)}, (l, seen)
        for want in ((px == -1), (px == W), (py == -1), (py == H)):      # exactly on the open ends: strictly outside
            assert bool(want.any())
    flat = loc[sel]
    assert bool(torch.isnan(flat).any()) and bool((flat >= FR.HUGE / 64).any()) and bool((flat <= -FR.HUGE / 64).any())
    # the placed samples are the same in the box form
    box = FR.locations(x, "box")
    t = len(FR.falloff_placements())
    q, h = np.divmod(np.arange(t), FR.M)
    assert FR._same(box[0, q, h][sel[0, q, h]], loc[0, q, h][sel[0, q, h]])


@pytest.mark.parametrize("name", ["slots", "falloff"])
def test_a_padded_token_lies_under_an_in_range_corner_of_every_level(name):
    x = FR.case(name)
    loc, sel = FR.sane(FR.locations(x, "point")), _selected(x)
    for l, (H, W) in enumerate(x["pyramid"]):
        ok, ys, xs, w, _, _ = R._geom(loc[:, :, :, l], H, W)
        found = False
        for k in range(4):
            pix = int(x["lsi"][l]) + ys[k].clamp(0, H - 1) * W + xs[k].clamp(0, W - 1)
            padded = ~torch.gather(x["keep"], 1, pix.flatten(1)).reshape(pix.shape)
            found |= bool((ok[k] & (w[k] > 0) & sel[:, :, :, l] & padded).any())
        assert found, l


@pytest.mark.parametrize("name", EXACT + ODD)
def test_masks_differ_at_both_ends_and_are_touched(name):
    x = FR.case(name)
    keep, B = x["keep"], x["keep"].shape[0]
    for b in range(1, B):
        assert keep[b, 0] != keep[b - 1, 0] and keep[b, -1] != keep[b - 1, -1]
    if x["exact"]:   # a selected sample sits exactly on token 0 and on token S - 1 of every image
        r0, r1 = FR.reference(x, "point", mask=False), FR.reference(x, "point", mask=True)
        for b in range(B):
            assert not torch.equal(r0["out"][b], r1["out"][b])
        loc, sel = FR.sane(FR.locations(x, "point")), _selected(x)
        H, W = x["pyramid"][-1]
        for b in range(B):
            first = (loc[b, :, :, 0] == torch.tensor([0.5 / x["pyramid"][0][1], 0.5 / x["pyramid"][0][0]], dtype=F64)).all(-1)
            last = (loc[b, :, :, -1] == torch.tensor([(W - 0.5) / W, (H - 0.5) / H], dtype=F64)).all(-1)
            assert bool((first & sel[b, :, :, 0]).any()) and bool((last & sel[b, :, :, -1]).any())


def test_straddling_cases_hold_two_images_in_a_workgroup_and_in_a_pair():
    """fp32: 4 consecutive queries per workgroup; bf16: 8 per workgroup, 2 per wave."""
    for name in ("slots", "slots_wave", "pairs", "bits_last_lds", "bits_memory"):
        B, Lq = FR.case(name)["off"].shape[:2]
        img = np.arange(B * Lq) // Lq
        for per in (4, 8, 2):
            pad = np.concatenate([img, np.full(-(B * Lq) % per, img[-1])]).reshape(-1, per)
            assert (pad.min(1) != pad.max(1)).any(), (name, per)
    B, Lq = FR.case("slots")["off"].shape[:2]
    assert (B * Lq) % 2 == 1                           # a dead last half
    assert -(-2 * 515 // 4) % 8 != 0                   # ragged XCD remap
    assert FR.case("threshold_1024")["off"].shape[1] == 1024 and FR.case("threshold_1025")["off"].shape[1] == 1025


def test_bits_cases_have_1024_and_1030_words():
    for name, words in (("bits_last_lds", 1024), ("bits_memory", 1030)):
        x = FR.case(name)
        S = x["keep"].shape[1]
        assert (S + 31) // 32 == words and x["value"].numel() * 4 < 100e6      # fp32 value on the device; the bf16 copy lives in another test
        # a selected sample of the second image, with a nonzero weight, lies on a token of the last mask word whose bit differs
        # between the images (token S - 1, placed by the builder): beyond word 1023 in bits_memory
        loc, sel = FR.sane(FR.locations(x, "point")), _selected(x)
        l = len(x["pyramid"]) - 1
        H, W = x["pyramid"][l]
        ok, ys, xs, w, _, _ = R._geom(loc[1, :, :, l], H, W)
        hit = False
        for k in range(4):
            pix = int(x["lsi"][l]) + ys[k].clamp(0, H - 1) * W + xs[k].clamp(0, W - 1)
            differs = (x["keep"][0] != x["keep"][1])[pix]
            hit |= bool((ok[k] & (w[k] > 0) & sel[1, :, :, l] & differs & (pix // 32 == words - 1)).any())
        assert hit, name


def test_containment_rows_are_some_but_not_all():
    x = FR.case("slots_wave")
    for form in ("point", "box"):
        for b, tok, h, c, what in FR.POISON:
            rows = FR.containment_rows(x, form, b, tok)[:, h]
            assert 0 < int(rows.sum()) < rows.numel(), (form, tok, int(rows.sum()))
            # rows whose in-range nonzero-weight corners use the token are among them
            v = x["value"].clone()
            v[b, tok, h, c] = 1e6
            y = dict(x, value=v)
            changed = (FR.reference(y, form)["out"] != FR.reference(x, form)["out"])[b].reshape(-1, FR.M, FR.D)[:, h, c]
            assert bool((rows | ~changed).all())


# ------------------------------------------------------------------------------------- the criteria see what they are for
def _config(mut):
    return dict(form="point", mask=mut in ("other_image_mask", "next_bit", "bias_on_padded"), bias=mut == "bias_on_padded")


@pytest.mark.parametrize("mut", FR.MUTATIONS)
def test_every_exact_case_rejects_a_forward_with_one_piece_wrong(mut):
    """Exact cases: the mutated float64 forward differs from the true one, and so do their bfloat16 images -- `equal` fails.
    (Where a mutation cannot apply -- one image, one level width, an even number of queries -- the case is skipped over;
    FR.applies.)  The cases above 32 768 tokens are left to the mask mutations, which is what they are for."""
    seen = 0
    for name in EXACT:
        x = FR.case(name)
        if not FR.applies(x, mut) or (name in FR.BITS_CASES and mut not in ("other_image_mask", "next_bit")):
            continue
        cfg = _config(mut)
        good, bad = FR.reference(x, **cfg)["out"], FR.reference(x, mut=mut, **cfg)["out"]
        assert not torch.equal(good, bad), (name, mut)
        assert not torch.equal(good.to(BF), bad.to(BF)), (name, mut, "bf16")
        seen += 1
    assert seen >= (2 if mut == "dead_half" else 4)


@pytest.mark.parametrize("mut", FR.MUTATIONS)
def test_a_budget_case_rejects_a_forward_with_one_piece_wrong(mut):
    rejected = []
    for name in ODD:
        x = FR.case(name)
        if not FR.applies(x, mut):
            continue
        cfg = _config(mut)
        r = FR.reference(x, geometry=True, **cfg)
        bad = FR.reference(x, mut=mut, **cfg)["out"]
        err = (bad - r["out"]).abs()
        rejected.append(bool((err > FR.bound_f32(r)).any()) and bool((err > 2 * FR.bound_bf16(r)).any()))
    assert any(rejected), mut


# ------------------------------------------------------------------------------------------------- the geometry term
def _fma_round(a32, n):
    """rn(a * n - 0.5) with one rounding: the product of a 24-bit and a small integer is exact in float64."""
    return (a32.double() * n - 0.5).float()


@pytest.mark.parametrize("name", ODD)
def test_delta_bounds_the_fp32_prologue(name):
    x = FR.case(name)
    W, H = FR._sizes(x, F64)
    worst = 0.0
    for form in ("point", "box"):
        dx, dy = FR.geometry_delta(x, form)
        exact = FR.locations(x, form)
        for order in ("rcp", "div"):
            loc32 = FR.locations(x, form, F32, order)
            for c, n, d in ((0, W, dx), (1, H, dy)):
                want = exact[..., c] * n - 0.5
                for got in (loc32[..., c] * n.float() - 0.5, _fma_round(loc32[..., c], n)):
                    assert got.dtype == F32
                    ratio = float(((got.double() - want).abs() / d).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (form, order, c, ratio)
    print(f"{name}: worst fp32 location error / delta {worst:.3f}")
    assert worst > 0.05     # the bound is not vacuous


@pytest.mark.parametrize("name", ODD)
def test_geometry_term_covers_a_forward_from_fp32_locations(name):
    """The float64 gather fed with the fp32 prologue's locations stays within the geometry term of the exact one."""
    x = FR.case(name)
    for form in ("point", "box"):
        r = FR.reference(x, form, mask=True, bias=True, geometry=True)
        y = dict(x)
        loc32 = FR.locations(x, form, F32, "rcp").double()
        kf = x["keep"].double()[:, :, None, None]
        v = (x["value"].double() + x["vbias"].double().view(1, 1, FR.M, FR.D)) * kf
        got = R.msda_forward_budget(v, y["pyramid"], y["lsi"].tolist(), loc32, FR.attention(x))["out"]
        ratio = R.worst_ratio(got, r["out"], r["geo"] + 4 * 2.0 ** -53 * (r["abs_out"] + r["abs_bias"]) * 64)
        print(f"{name} [{form}]: worst error from fp32 locations / geometry term {ratio:.3f}")
        assert ratio <= 1.0


def test_bf16_budget_on_an_emulation_of_the_kernel_arithmetic():
    """fp32 geometry, weight x attention rounded to bfloat16, fp32 accumulation, bfloat16 output: inside bound_bf16 on the
    budget cases and equal to the rounded float64 result on the exact ones."""
    for name in ("slots", "pairs", "dense", "odd_37"):
        x = FR.case(name)
        loc, attn = FR.sane(FR.locations(x, "point", F32, "rcp")), FR.attention(x, F32)
        B, Lq = loc.shape[:2]
        S = x["value"].shape[1]
        vflat = x["value"].reshape(B * S * FR.M, FR.D)
        acc = torch.zeros(B, Lq, FR.M, FR.D, dtype=F32)
        for l, (H, W) in enumerate(x["pyramid"]):
            for p in range(loc.shape[4]):
                px, py = loc[:, :, :, l, p, 0] * float(W) - 0.5, loc[:, :, :, l, p, 1] * float(H) - 0.5
                ok, ys, xs, _, _, _ = R._geom(loc[:, :, :, l, p].double(), H, W)
                lw, lh = px - px.floor(), py - py.floor()
                for k, w in enumerate(((1 - lh) * (1 - lw), (1 - lh) * lw, lh * (1 - lw), lh * lw)):
                    wa = torch.where(ok[k], w * attn[:, :, :, l, p], torch.zeros_like(w)).to(BF).float()
                    pix = int(x["lsi"][l]) + ys[k].clamp(0, H - 1) * W + xs[k].clamp(0, W - 1)
                    acc = acc + wa[..., None] * vflat[R._rows(B, S, FR.M, pix)].reshape(B, Lq, FR.M, FR.D)
        got = acc.to(BF).reshape(B, Lq, -1)
        r = FR.reference(x, "point", geometry=not x["exact"])
        if x["exact"]:
            assert torch.equal(got, r["out"].to(BF)), name
        else:
            FR.check(f"{name} [bf16 emulation]", got, r, FR.bound_bf16(r))
