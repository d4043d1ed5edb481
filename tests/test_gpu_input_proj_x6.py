"""GPU (-m gpu): the grouped, K-split input projections (egtr_amd/csrc/input_proj_x6.hip) and the token GroupNorm that sums their
slabs (egtr_amd/csrc/elementwise.hip, gn_partial_tokens<float, true>), in the manner of tests/test_gpu_backbone_x6.py and
tests/test_gpu_token_x6.py: paired operands whose leading products cancel, every bar computed in the test from the fp64
restatement of the operands the kernel multiplies (bar = sqrt(E_model E_loss)), teeth tests that remove one piece, per-output
bounds on adversarial operands.  The shapes are the smallest at which each thing can go wrong: one ragged 64-row tile, several
tiles plus a ragged one, odd and even planes for the stride-2 gather (every border case), two images, S_l forced to 1 and 2 and
the plan's own, and one case at the real C = 2048 where K = 18 432 is cut into 36 tap-aligned pieces.

The K ranges of a level are summed here as the statistics pass sums them: in fp32, slab 0 first."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import helpers as H
from groupnorm_restated import sum_slabs as _sum_slabs     # fp32, slab order 0, 1, ...: gn_partial_tokens<float, true>'s
from test_gpu_backbone_x6 import ADVERSARIAL, Case, _adversarial, _check_per_output, _check_six_terms, _check_teeth, _gen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAMILIES = ["act", "wgt"]


def _plan(cases):
    from egtr_amd import ops
    return ops.input_proj_x6_plan([c.rows for c in cases], [c.K for c in cases], [c.C if c.conv else 0 for c in cases])[0]


def _launch(cases, operands, splits):
    """one launch over ``cases`` with the given (a, w) per case -> the summed product of every case in its op's layout"""
    from egtr_amd import ops
    maps = [c.as_map(a) for c, (a, _) in zip(cases, operands)]
    wts = [ops.input_proj_x6_weights(c.as_conv_weight(w)) for c, (_, w) in zip(cases, operands)]
    slabs, got, shapes = ops.input_proj_x6(maps, wts, [c.conv for c in cases], splits=splits)
    assert got == list(splits) and [tuple(s.shape[:1]) for s in slabs] == [(v,) for v in splits]
    return [c.from_tokens(_sum_slabs(s)) for c, s in zip(cases, slabs)]


def _split_choices(case):
    """S forced to 1 and 2 where the K stages divide, and the plan's own"""
    own = _plan([case])[0]
    return sorted({s for s in (1, 2) if (case.K // 32) % s == 0} | {own}), own


class PlainCase(Case):
    conv = False

    def __init__(self, a_gen, w_gen, only_plan=False):
        self.a, self.w = a_gen.to(DEV), w_gen.to(DEV)
        self.rows, self.K, self.C = self.a.shape[0], self.a.shape[1], self.a.shape[1]
        self.only_plan = only_plan
        self.name = f"input_proj plain M={self.rows} K={self.K}"

    @staticmethod
    def op(a, w):
        return a @ w.t()

    def as_map(self, a):
        return a.contiguous().view(1, a.shape[0], 1, a.shape[1]).permute(0, 3, 1, 2)     # [1, K, M, 1], channels-last memory

    @staticmethod
    def as_conv_weight(w):
        return w[:, :, None, None]

    @staticmethod
    def from_tokens(y):
        return y.reshape(-1, 256)

    def runs(self, a, w):
        choices, own = _split_choices(self)
        if self.only_plan:
            choices = [own]
        return [(f"S={s}" + (" (plan)" if s == own else ""), _launch([self], [(a, w)], [s])[0]) for s in choices]


class Conv3s2Case(Case):
    conv = True

    def __init__(self, a_gen, w_gen, only_plan=False):
        self.a = a_gen.to(DEV).permute(0, 3, 1, 2)                       # [B, C, H, W], channels-last memory
        self.w = w_gen.to(DEV).permute(0, 3, 1, 2).contiguous()          # [256, C, 3, 3]
        self.B, self.C, self.H, self.W = self.a.shape
        self.Ho, self.Wo = (self.H - 1) // 2 + 1, (self.W - 1) // 2 + 1
        self.rows, self.K = self.B * self.Ho * self.Wo, 9 * self.C
        self.only_plan = only_plan
        self.name = f"input_proj 3x3/s2 C={self.C} {tuple(self.a.shape)}"

    @staticmethod
    def op(a, w):
        return F.conv2d(a, w, None, stride=2, padding=1)

    @staticmethod
    def as_map(a):
        return a.contiguous(memory_format=torch.channels_last)

    @staticmethod
    def as_conv_weight(w):
        return w

    def from_tokens(self, y):
        return y.reshape(self.B, self.Ho, self.Wo, 256).permute(0, 3, 1, 2)

    runs = PlainCase.runs


class Grouped(Case):
    """case ``i`` of four levels multiplied in ONE launch: the other levels keep their stored operands"""

    def __init__(self, cases, i, splits):
        self.cases, self.i, self.splits = cases, i, splits
        c = cases[i]
        self.a, self.w, self.op, self.K = c.a, c.w, c.op, c.K
        self.name = f"grouped[{i}] {c.name} splits {splits}"

    def runs(self, a, w):
        ops_ = [(c.a, c.w) for c in self.cases]
        ops_[self.i] = (a, w)
        return [("grouped", _launch(self.cases, ops_, self.splits)[self.i])]


def _plain_case(family, M, K, **kw):
    return PlainCase(*H.paired_operands(family, (M, K), (256, K), _gen("ip-plain", family, M, K)), **kw)


def _conv_case(family, C, size, **kw):
    B, Hh, Ww = size
    return Conv3s2Case(*H.paired_operands(family, (B, Hh, Ww, C), (256, 3, 3, C), _gen("ip-conv", family, C, *size)), **kw)


# ---- 1. products against fp64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("M,K", [(37, 64), (160, 64), (2399, 64), (160, 1024)])
def test_plain_level_keeps_all_six_terms(family, M, K):
    """one ragged tile, full tiles + a ragged one, several tiles; one K stage per unit and many; S = 1, 2 and the plan's"""
    _check_six_terms(_plain_case(family, M, K), family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("plane", [(5, 7), (6, 8), (19, 32)])
def test_strided_3x3_level_keeps_all_six_terms(family, B, plane):
    """odd and even extents (every border case of the stride-2 gather), per-image addressing, pieces that straddle taps (S forced
    to 1 and 2) and tap-aligned ones (the plan's)"""
    _check_six_terms(_conv_case(family, 64, (B, *plane)), family)


@pytest.mark.parametrize("family", FAMILIES)
def test_strided_3x3_level_at_the_real_channel_count(family):
    """C = 2048 on the 5 x 7 plane: K = 18 432 in 36 or more tap-aligned pieces"""
    case = _conv_case(family, 2048, (1, 5, 7), only_plan=True)
    (own,) = _plan([case])
    assert own >= 36 and 2048 % (case.K // own) == 0
    _check_six_terms(case, family)


@pytest.mark.parametrize("family", FAMILIES)
def test_four_levels_in_one_launch_keep_all_six_terms(family):
    cases = [_plain_case(family, 2399, 64), _plain_case(family, 160, 128), _plain_case(family, 37, 64),
             _conv_case(family, 64, (1, 6, 8))]
    for splits in (_plan(cases), [1, 2, 1, 2]):
        for i in range(4):
            _check_six_terms(Grouped(cases, i, splits), family)


# ---- 2. teeth -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind", ["plain", "3x3"])
def test_bar_is_exceeded_when_one_piece_is_removed(family, kind):
    _check_teeth(_plain_case(family, 160, 1024) if kind == "plain" else _conv_case(family, 64, (2, 6, 8)), family)


# ---- 3. per-output bound, K the FULL reduction length ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ADVERSARIAL)
@pytest.mark.parametrize("level", ["plain", "3x3"])
def test_per_output_bound_on_adversarial_operands(kind, level):
    """|y - ref| <= (6 K / 16 + 4) 2^-23 sum |w| |a|.  The split form's own bound, (6 K_s / 16 + 4 + S) 2^-23 sum |w| |a|, is not
    larger whenever S <= 6 (K - K_s) / 16, which tests/test_input_proj_plan_cpu.py asserts of every plan."""
    if level == "plain":
        case = PlainCase(*_adversarial(kind, (97, 256), (256, 256), _gen("adv-ip", kind, 256)))
    else:
        case = Conv3s2Case(*_adversarial(kind, (2, 6, 8, 64), (256, 3, 3, 64), _gen("adv-ip3", kind, 64)))
    _check_per_output(case, kind)


# ---- 4. padding ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [(5, 7), (6, 8)])
@pytest.mark.parametrize("live", [0, 1])
def test_taps_outside_the_image_contribute_zeros_and_every_slab_element_is_written(plane, live):
    """The feature map lies inside a larger allocation whose rows before and after it, and the OTHER image of the batch, hold
    1e30: a tap that read a neighbouring row, image or allocation would show at once.  The workspace is NaN before the call."""
    from egtr_amd import ops
    Hh, Ww = plane
    C, B = 64, 2
    g = _gen("ip-pad", Hh, Ww, live)
    n, guard = B * Hh * Ww * C, 4 * Ww * C
    buf = torch.full((n + 2 * guard,), 1e30)
    a = buf[guard:guard + n].view(B, Hh, Ww, C)
    a[live] = torch.randn(Hh, Ww, C, generator=g)
    w = torch.randn(256, 3, 3, C, generator=g) / (9 * C) ** 0.5
    dbuf = buf.to(DEV)
    fm = dbuf[guard:guard + n].view(B, Hh, Ww, C).permute(0, 3, 1, 2)
    assert fm.is_contiguous(memory_format=torch.channels_last) and fm.data_ptr() % 16 == 0
    wc = w.permute(0, 3, 1, 2).contiguous()
    ref = F.conv2d(a[live:live + 1].permute(0, 3, 1, 2).double(), wc.double(), None, stride=2, padding=1)
    mag = F.conv2d(a[live:live + 1].permute(0, 3, 1, 2).double().abs(), wc.double().abs(), None, stride=2, padding=1)
    Ho, Wo = ref.shape[-2:]
    wt = ops.input_proj_x6_weights(wc.to(DEV))
    for s in (1, 2, 9, 18):
        slabs = [torch.full((s, B, Ho * Wo, 256), float("nan"), device=DEV)]
        ops.input_proj_x6([fm], [wt], [True], splits=[s], slabs=slabs)
        assert not bool(torch.isnan(slabs[0]).any()), f"S={s}: a slab element was left unwritten"
        y = _sum_slabs(slabs[0])[live].view(1, Ho, Wo, 256).permute(0, 3, 1, 2).cpu().double()
        e = (y - ref).abs()
        assert bool((e <= (6 * 9 * C / 16 + 4) * 2.0 ** -23 * mag).all()), (s, float(e.max()))


# ---- 5. GroupNorm on slabs -------------------------------------------------------------------------------------------------------------
GN_SHAPES = [(19, 33), (10, 17), (5, 9), (3, 3)]


def _projs():
    torch.manual_seed(9)
    projs = nn.ModuleList([nn.Sequential(nn.Conv2d(8, 256, 1), nn.GroupNorm(32, 256)) for _ in GN_SHAPES])
    with torch.no_grad():
        for p in projs:
            p[0].bias.normal_()
            p[1].weight.normal_()
            p[1].bias.normal_()
    return projs


@pytest.mark.parametrize("S", [1, 2, 5])
def test_groupnorm_sums_the_slabs_in_order(S):
    from egtr_amd import ops
    projs = _projs()
    g = torch.Generator().manual_seed(50 + S)
    xs = [3.0 * torch.randn(2, h * w, 256, generator=g) + 1.5 for h, w in GN_SHAPES]
    slabs = []
    for x in xs:      # a random split of x: S - 1 random slabs, slab 0 the rest
        rest = [2.0 * torch.randn(x.shape, generator=g) for _ in range(S - 1)]
        first = x.clone()
        for r in rest:
            first = first - r
        slabs.append(torch.stack([first] + rest).to(DEV))
    total64 = [s.cpu().double().sum(0) for s in slabs]
    with torch.no_grad():
        want = torch.cat([F.group_norm(t.transpose(1, 2) + p[0].bias.double().view(1, -1, 1), 32, p[1].weight.double(),
                                       p[1].bias.double(), p[1].eps).transpose(1, 2) for p, t in zip(projs, total64)], 1)
    dprojs = projs.to(DEV)
    with torch.no_grad():
        sums32 = [_sum_slabs(s) for s in slabs]
        plain = ops.input_proj_groupnorm_tokens(sums32, dprojs)
        work = [s.clone() for s in slabs]
        got = ops.input_proj_groupnorm_token_slabs(work, dprojs)
        again = ops.input_proj_groupnorm_token_slabs([s.clone() for s in slabs], dprojs)
    assert got.shape == want.shape == plain.shape
    err = float((got.cpu().double() - want).abs().max())
    print(f"\n[gn slabs S={S}] max |got - fp64| {err:.3g}; equal to the plain entry on the fp32 sum: {torch.equal(got, plain)}")
    assert torch.equal(got, again), "two calls on the same slabs must be bit-identical"
    if S == 1:
        assert torch.equal(got, plain)
    assert err < 2e-5
    for wk, s32 in zip(work, sums32):     # the sum is left in slab 0, in slab order
        assert torch.equal(wk[0], s32)


# ---- 6. the whole route against the vendor route and fp64 -----------------------------------------------------------------------------
def test_route_against_the_vendor_route_and_fp64_eager_and_graph_replayed():
    from egtr_amd import ops
    torch.manual_seed(11)
    chans, planes, B = [64, 128, 256], [(19, 33), (10, 17), (5, 9)], 2
    projs = nn.ModuleList([nn.Sequential(nn.Conv2d(c, 256, 1), nn.GroupNorm(32, 256)) for c in chans]
                          + [nn.Sequential(nn.Conv2d(256, 256, 3, stride=2, padding=1), nn.GroupNorm(32, 256))])
    with torch.no_grad():
        for p in projs:
            p[0].bias.normal_()
            p[1].weight.normal_()
            p[1].bias.normal_()
    maps = [torch.randn(B, c, h, w) for c, (h, w) in zip(chans, planes)]
    with torch.no_grad():
        want = []
        for l, p in enumerate(projs):
            x = maps[min(l, len(maps) - 1)].double()
            y = F.conv2d(x, p[0].weight.double(), p[0].bias.double(), p[0].stride, p[0].padding)
            want.append(F.group_norm(y, 32, p[1].weight.double(), p[1].bias.double(), p[1].eps).flatten(2).transpose(1, 2))
        want = torch.cat(want, 1)
    dprojs = projs.to(DEV)
    dmaps = [m.to(DEV).contiguous(memory_format=torch.channels_last) for m in maps]
    with torch.no_grad():
        assert ops.input_proj_x6_supported(dmaps, dprojs)
        got, shapes = ops.input_proj_x6_groupnorm(dmaps, dprojs)
        assert shapes == planes + [(3, 5)]
        toks = []                                           # the vendor route of DeformableDetrModel.forward
        for fm, p in zip(dmaps, dprojs):
            b_, c_, h_, w_ = fm.shape
            toks.append(torch.mm(fm.permute(0, 2, 3, 1).reshape(-1, c_), p[0].weight.view(256, c_).t()).view(b_, h_ * w_, -1))
        y = F.conv2d(dmaps[-1], dprojs[3][0].weight.contiguous(memory_format=torch.channels_last), None, (2, 2), (1, 1))
        toks.append(y.permute(0, 2, 3, 1).reshape(B, -1, 256))
        vendor = ops.input_proj_groupnorm_tokens(toks, dprojs)
    e_new = float((got.cpu().double() - want).abs().max())
    e_vendor = float((vendor.cpu().double() - want).abs().max())
    print(f"\n[route] max error against fp64: grouped x6 {e_new:.3g}, vendor fp32 {e_vendor:.3g}")
    assert got.shape == want.shape
    assert e_new <= 2.5 * e_vendor, (e_new, e_vendor)
    # captured and replayed: bit for bit the eager result
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        ops.input_proj_x6_groupnorm(dmaps, dprojs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        replayed, _ = ops.input_proj_x6_groupnorm(dmaps, dprojs)
    replayed.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(replayed, got)


# ---- 7. model level --------------------------------------------------------------------------------------------------------------------
def test_real_resnet50_model_with_the_grouped_route_on_and_off(monkeypatch):
    """The product model with the in-repo ResNet-50 at 128 x 160: the grouped route against its off-twin (ops.GEMM_SPLIT_BF16
    off: the vendor fp32 products), within the 1e-3 that test_real_resnet50_product_routes_vs_oracle holds each route to."""
    from egtr_amd import ops
    import test_gpu_model as TM
    model, _, _ = TM._real_backbone_model(30, 2, 2)
    torch.manual_seed(5)
    pv = torch.randn(2, 3, 128, 160)
    pm = torch.ones(2, 128, 160, dtype=torch.long)
    pm[1, 128 - 19:, :] = 0
    pm[1, :, 160 - 37:] = 0
    pv[1] = pv[1] * pm[1][None].float()
    calls = []
    real = ops.input_proj_x6_groupnorm
    monkeypatch.setattr(ops, "input_proj_x6_groupnorm", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    on = TM._heads_logits(model, pv.to(DEV), pm.to(DEV), False)
    assert len(calls) == 1, "the inference forward must take the grouped route"
    monkeypatch.setattr(ops, "GEMM_SPLIT_BF16", False)
    off = TM._heads_logits(model, pv.to(DEV), pm.to(DEV), False)
    assert len(calls) == 1, "the off-twin must not"
    td = model.triplet_dist
    for k in ("logits", "pred_boxes", "conn_logits"):
        d = float((on[k] - off[k]).abs().max())
        print(f"\n[model] max |on - off| {k}: {d:.3g}")
        assert d < 1e-3, k
    a = TM.Hh.rel_mlp_from_logits(on["rel_logits"].cpu(), on["logits"].cpu(), td.cpu())
    b = TM.Hh.rel_mlp_from_logits(off["rel_logits"].cpu(), off["logits"].cpu(), td.cpu())
    assert float((a - b).abs().max()) < 1e-3
