"""GPU (-m gpu): the ARITHMETIC of the backbone's split-bf16 kernels -- the bottleneck tail (csrc/conv_tail_x6.hip), the 3x3
convolution in its three kernels and five variants and the strided 1x1 projection (csrc/conv3x3_x6.hip), the fused stem
(csrc/stem_x6.hip) -- and the weight streams they read (csrc/xs_split.hip, ops.conv3x3_weights, ops.stem_weights).

Their claim is fp32-level accuracy from six bf16 cross terms (x6::mfma6).  On N(0, 1) operands a kernel that loses one of the three
small terms is only 3-5x further from fp64 than a correct one that accumulates K = 4608 products in fp32, so no tolerance can
tell them apart.  Here the operands are built so that it can (helpers.paired_operands, checked on the host by
tests/test_split_arith_cpu.py): the leading products cancel in adjacent k pairs and the result is carried by the small pieces.

  * every bar of the paired-operand tests is computed IN the test from the fp64 restatement of the split arithmetic
    (helpers.split_error_model): E_model = relative Frobenius error of the six-term sum, E_loss = the smallest such error of a
    five-term sum (over the two small terms the family resolves; its third is exactly zero by construction, and the other family
    resolves it), bar = sqrt(E_model E_loss), about 10x from either.  The plain fp32 route has to meet the bar on the same
    operands first, or the inputs are at fault;
  * the teeth tests feed the kernels operands with one piece REMOVED and require the bar to be exceeded;
  * the per-output tests hold |y - ref| <= (6 K / 16 + 4) 2^-23 sum |w| |a| on operands far from N(0, 1): the worst case of a
    chain of 6 K / 16 fp32 accumulations (unit round-off 2^-23: a truncating accumulator is covered) plus the three dropped terms
    (each <= 2^-24 |w| |a|, a fourth unit for the pieces' own representation); fp32 denormal inputs add the absolute 2^-126 K
    of tests/test_gpu_pinning.py (the matrix pipe may flush denormal pieces).  The vendor fp32 route meets the same bound.
"""
import pytest
import torch
import torch.nn.functional as F

import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# every (C, stride) -> variants the dispatcher serves: the list of tests/test_gpu_kernels.py::test_conv3x3_x6_matches_fp64_convolution
CONV3_VARIANTS = {(64, 1): (0, 1, 2, 3, 4), (128, 1): (0, 1, 2, 3, 4), (256, 1): (0, 1, 3), (512, 1): (0, 1),
                  (128, 2): (0, 1), (256, 2): (0, 1), (512, 2): (0, 1)}
TAIL_KN = [(64, 256), (128, 512), (256, 1024), (512, 2048), (64, 128), (256, 384), (64, 64), (256, 192)]
STRIDED_CN = [(256, 512), (512, 1024), (1024, 2048), (256, 128)]
FAMILIES = ["act", "wgt"]


def _tail_tiles(K, N):
    """every tile the dispatcher accepts (tests/test_gpu_kernels.py::test_conv1x1_tail_matches_fp64_product)"""
    return [(0, 0)] + ([(32, 128)] if N % 128 == 0 else []) + ([(32, 256)] if N % 256 == 0 else []) \
        + ([(64, 128)] if K <= 256 and N % 128 == 0 else []) + ([(64, 256)] if K <= 256 and N % 256 == 0 else [])


def _gen(*key):
    seed = 0
    for v in key:
        seed = seed * 1009 + (sum(map(ord, v)) if isinstance(v, str) else int(v))
    return torch.Generator().manual_seed(seed % (2 ** 31))


# ---- the four kernels as (operands in generation layout [..., channel]) -> (kernel operands, fp64 operator, runs, fp32 route) ----
class Case:
    """a, w: the kernel's fp32 operands on the device; op(a, w): the linear operator in the dtype of its arguments; post: what
    the kernel applies behind it; runs(a, w): [(label, kernel output in op's layout)]; K: products per output the kernel walks."""
    post = staticmethod(lambda t: t)
    post_bound = staticmethod(lambda t: t)
    a_split = w_split = None      # helpers.split_error_model's defaults: activation = truncation, weight = nearest even

    def fp32(self, a, w):
        return self.post(self.op(a, w))


class TailCase(Case):
    def __init__(self, a_gen, w_gen):
        self.a, self.w = a_gen.to(DEV), w_gen.to(DEV)
        self.K, self.N = self.w.shape[1], self.w.shape[0]
        self.name = f"tail K={self.K} N={self.N} M={self.a.shape[0]}"

    @staticmethod
    def op(a, w):
        return a @ w.t()

    def runs(self, a, w):
        from egtr_amd import ops
        wxs = ops.xs_split(w, weights=True)
        return [(f"tile {t}", ops.conv1x1_tail(a, None, wxs, None, None, self.N, relu_in=False, relu_out=False, tile=t))
                for t in _tail_tiles(self.K, self.N)]


class Conv3Case(Case):
    def __init__(self, a_gen, w_gen, stride, variants):
        self.a = a_gen.to(DEV).permute(0, 3, 1, 2)                       # [B, C, H, W], channels-last memory
        self.w = w_gen.to(DEV).permute(0, 3, 1, 2).contiguous()          # [N, C, 3, 3]
        self.C, self.stride, self.variants = self.w.shape[1], stride, variants
        self.K = 9 * self.C
        self.name = f"conv3x3 C={self.C} stride={stride} {tuple(self.a.shape)}"

    def op(self, a, w):
        return F.conv2d(a, w, None, stride=self.stride, padding=1)

    def runs(self, a, w):
        from egtr_amd import ops
        a = a.contiguous(memory_format=torch.channels_last)
        assert ops.conv3x3_supported(a, self.C, self.stride)
        return [(f"variant {v}", ops.conv3x3(a, ops.conv3x3_weights(w, self.stride, v), self.C, self.stride, v)) for v in self.variants]


class StridedCase(Case):
    def __init__(self, a_gen, w_gen, stride):
        self.a = a_gen.to(DEV).permute(0, 3, 1, 2)                       # [B, C, H, W], channels-last memory
        self.w = w_gen.to(DEV)                                           # [N, C]
        self.N, self.K, self.stride = self.w.shape[0], self.w.shape[1], stride
        self.name = f"conv1x1 strided C={self.K} N={self.N} stride={stride} {tuple(self.a.shape)}"

    def op(self, a, w):
        return F.conv2d(a, w[:, :, None, None], None, stride=self.stride)

    def runs(self, a, w):
        from egtr_amd import ops
        a = a.contiguous(memory_format=torch.channels_last)
        assert ops.conv1x1_strided_supported(a, self.N, self.stride)
        y = ops.conv1x1_strided(a, ops.xs_split(w.contiguous(), weights=True), self.N, self.stride)
        B, _, Hh, Ww = a.shape
        Ho, Wo = (Hh - 1) // self.stride + 1, (Ww - 1) // self.stride + 1
        return [("", y.view(B, Ho, Wo, self.N).permute(0, 3, 1, 2))]


class StemCase(Case):
    """Channels 0 and 1 of a pixel are the adjacent k pair; channel 2 carries activations and ZERO weights.  The kernel keeps its
    ReLU + 3x3/2 max-pool (zero shift), so every restatement goes through the same two."""
    K = 224                                                              # 7 rows x 8 taps x 4 channels: what the kernel walks
    post = staticmethod(lambda t: F.max_pool2d(torch.relu(t), 3, 2, 1))
    post_bound = staticmethod(lambda t: F.max_pool2d(t, 3, 2, 1))        # |max relu y - max relu r| <= max |y - r| over the window

    def __init__(self, a_gen, w_gen):
        self.a = a_gen.to(DEV).permute(0, 3, 1, 2).contiguous()          # [B, 3, H, W] NCHW
        self.w = w_gen.to(DEV).permute(0, 3, 1, 2).contiguous()          # [64, 3, 7, 7]
        self.name = f"stem {tuple(self.a.shape)}"

    @staticmethod
    def op(a, w):
        return F.conv2d(a, w, None, stride=2, padding=3)

    def runs(self, a, w):
        from egtr_amd import ops
        a = a.contiguous()
        assert ops.stem_fused_supported(a, w)
        return [("", ops.stem_fused(a, ops.stem_weights(w), torch.zeros(64, device=DEV)))]


def _stem_paired(family, B, Hh, Ww, g):
    a2, w2 = H.paired_operands(family, (B, Hh, Ww, 2), (64, 7, 7, 2), g)
    a = torch.cat([a2, torch.randn(B, Hh, Ww, 1, generator=g)], dim=-1)
    w = torch.cat([w2, torch.zeros(64, 7, 7, 1)], dim=-1)
    return a, w


def _tail_case(family, K, N, M):
    return TailCase(*H.paired_operands(family, (M, K), (N, K), _gen("tail", family, K, N, M)))


def _conv3_case(family, C, stride, size, variants=None):
    B, Hh, Ww = size
    a, w = H.paired_operands(family, (B, Hh, Ww, C), (C, 3, 3, C), _gen("conv3", family, C, stride, *size))
    return Conv3Case(a, w, stride, CONV3_VARIANTS[(C, stride)] if variants is None else variants)


def _strided_case(family, C, N, stride, size):
    B, Hh, Ww = size
    return StridedCase(*H.paired_operands(family, (B, Hh, Ww, C), (N, C), _gen("strided", family, C, N, stride, *size)), stride)


def _stem_case(family, size):
    return StemCase(*_stem_paired(family, *size, _gen("stem", family, *size)))


# ---- item 2: paired operands, bar from the fp64 restatement ---------------------------------------------------------------------
def _model(case, family):
    ref, e_model, e_loss = H.split_error_model(case.op, case.a, case.w, post=case.post, lost=H.RESOLVED_TERMS[family],
                                               a_split=case.a_split, w_split=case.w_split)
    return ref, e_model, e_loss, (e_model * e_loss) ** 0.5


def _check_six_terms(case, family):
    ref, e_model, e_loss, bar = _model(case, family)
    e32 = H.rel_fro(case.fp32(case.a, case.w), ref)
    print(f"\n[six-terms {family}] {case.name}: E_model {e_model:.3g} E_loss {e_loss:.3g} bar {bar:.3g} fp32 route {e32:.3g}")
    assert e_loss >= 50 * e_model, "input health: a lost term must stand out of the six-term model"
    assert e32 <= bar, "input health: the plain fp32 route must itself meet the bar"
    worst = 0.0
    for label, y in case.runs(case.a, case.w):
        assert y.shape == ref.shape, (y.shape, ref.shape)
        err = H.rel_fro(y, ref)
        print(f"    {label}: err_kernel {err:.3g} = {err / e_model:.2f} x E_model")
        assert err <= bar, (case.name, label, err, bar)
        worst = max(worst, err / e_model)
    return worst


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("K,N", TAIL_KN)
@pytest.mark.parametrize("M", [37, 2399])
def test_tail_keeps_all_six_terms(family, K, N, M):
    """egtr_conv1x1_tail_x6_f32, no shift / bias / shortcut, both ReLUs off, every tile: relative Frobenius error against fp64 within
    sqrt(E_model E_loss) of the case."""
    _check_six_terms(_tail_case(family, K, N, M), family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("C,stride", sorted(CONV3_VARIANTS))
@pytest.mark.parametrize("size", [(2, 17, 33), (1, 5, 7)])
def test_conv3x3_keeps_all_six_terms_in_every_variant(family, C, stride, size):
    """egtr_conv3x3_x6_f32: the two-wave, K-split and phased kernels and each weight-stream reordering (every variant of every
    (C, stride)), at a ragged size and one below a tile.  Channel pairs (2i, 2i + 1) of a tap are adjacent k."""
    _check_six_terms(_conv3_case(family, C, stride, size), family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("C,N", STRIDED_CN)
@pytest.mark.parametrize("stride", [1, 2])
def test_conv1x1_strided_keeps_all_six_terms(family, C, N, stride):
    _check_six_terms(_strided_case(family, C, N, stride, (2, 17, 33)), family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("size", [(2, 61, 83), (1, 224, 320)])
def test_stem_keeps_all_six_terms(family, size):
    """egtr_stem_conv7x7_pool_x6_f32 with zero shift: the six-term, five-term and fp64 restatements each go through the same
    ReLU + 3x3/2 max-pool before the errors are taken, and the health conditions are checked on the pooled values."""
    _check_six_terms(_stem_case(family, size), family)


# ---- item 3: the metric resolves ONE term on the real matrix pipe ----------------------------------------------------------------
def _check_teeth(case, family):
    """Operands with one piece removed, against the fp64 result of the INTACT operands: exactly a lost term.  "wgt": weights
    w - w_lo (loses w_lo a_hi) and, for nearest-even weights, w - w_mid - w_lo (also w_mid a_hi, w_mid a_mid); "act": activations
    a - a_lo (w_hi a_lo).  A case with split functions of its own (the weight gradient: a is g, w is x) is damaged by those."""
    ref, e_model, e_loss, bar = _model(case, family)
    assert e_loss >= 50 * e_model
    intact = max(H.rel_fro(y, ref) for _, y in case.runs(case.a, case.w))
    assert intact <= bar
    if family == "wgt":
        hi, mid, lo = (case.w_split or H.split3_rne)(case.w)
        damaged = [("w - w_lo", case.a, hi + mid)] + ([("w - w_mid - w_lo", case.a, hi)] if case.w_split is None else [])
    else:
        hi, mid, lo = (case.a_split or H.split3_trunc)(case.a)
        damaged = [("a - a_lo", hi + mid, case.w)]
    assert torch.equal((hi + mid).double(), hi.double() + mid.double())               # the removal is exact in fp32
    assert float(lo.abs().max()) > 0
    for what, a, w in damaged:
        for label, y in case.runs(a, w):
            err = H.rel_fro(y, ref)
            print(f"\n[teeth {family}] {case.name} {label} {what}: err {err:.3g} vs bar {bar:.3g} (intact {intact:.3g})")
            assert err > bar, (case.name, what, label, err, bar)


@pytest.mark.parametrize("family", FAMILIES)
def test_tail_bar_is_exceeded_when_one_piece_is_removed(family):
    _check_teeth(_tail_case(family, 256, 1024, 2399), family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("C,stride", [(64, 1), (256, 1), (512, 2)])
def test_conv3x3_bar_is_exceeded_when_one_piece_is_removed(family, C, stride):
    """one (C, stride) per kernel: two-wave (64), K-split / phased (256, 512), all their variants"""
    _check_teeth(_conv3_case(family, C, stride, (2, 17, 33)), family)


@pytest.mark.parametrize("family", FAMILIES)
def test_conv1x1_strided_bar_is_exceeded_when_one_piece_is_removed(family):
    _check_teeth(_strided_case(family, 512, 1024, 2, (2, 17, 33)), family)


@pytest.mark.parametrize("family", FAMILIES)
def test_stem_bar_is_exceeded_when_one_piece_is_removed(family):
    _check_teeth(_stem_case(family, (2, 61, 83)), family)


# ---- item 4: per-output bounds on operands far from N(0, 1) ---------------------------------------------------------------------
ADVERSARIAL = ["out-scale", "in-scale", "large", "half-zero", "denormal"]


def _adversarial(kind, a_shape, w_shape, g):
    """(a [..., C], w [N, ..., C]) in generation layout.  out-scale / in-scale: every output channel / every input channel of w
    (and, in-scale, of a) at its own power of two 2^-20 .. 2^20, as folded batch-norm scales do to real weights; large:
    activations x 1e4; half-zero: post-ReLU activations; denormal: fp32 denormals and, every third pixel, values whose last
    piece is denormal."""
    fan_in = 1
    for d in w_shape[1:]:
        fan_in *= d
    a = torch.randn(*a_shape, generator=g)
    w = torch.randn(*w_shape, generator=g) / fan_in ** 0.5
    C, N = a_shape[-1], w_shape[0]
    p2 = lambda n: torch.pow(2.0, torch.randint(-20, 21, (n,), generator=g).float())
    if kind == "out-scale":
        w = w * p2(N).view(N, *([1] * (w.dim() - 1)))
    elif kind == "in-scale":
        w = w * p2(C)
        a = a * p2(C)
    elif kind == "large":
        a = a * 1e4
    elif kind == "half-zero":
        a = torch.relu(a)
    elif kind == "denormal":
        a = a * 1e-39
        rows = a.view(-1, C)
        rows[::3] = rows[::3] * 1e4
    else:
        raise ValueError(kind)
    return a, w


def _check_per_output(case, kind):
    ref = case.post(case.op(case.a.double(), case.w.double()))
    mag = case.op(case.a.double().abs(), case.w.double().abs())
    bound = case.post_bound((6 * case.K / 16 + 4) * 2.0 ** -23 * mag + (2.0 ** -126 * case.K if kind == "denormal" else 0.0))
    unit = case.post_bound(2.0 ** -24 * mag)
    outs = [("vendor fp32", case.fp32(case.a, case.w))] + case.runs(case.a, case.w)
    for label, y in outs:
        assert y.shape == ref.shape and bool(torch.isfinite(y).all()), (case.name, label)
        e = (y.double() - ref).abs()
        ok = unit > 0
        ratio = float((e[ok] / unit[ok]).max()) if kind != "denormal" else float("nan")
        print(f"\n[per-output {kind}] {case.name} {label}: max |y - ref| / (2^-24 mag) = {ratio:.2f}, "
              f"bound at {2 * (6 * case.K / 16 + 4):.0f}")
        assert bool((e <= bound).all()), (case.name, kind, label, float((e / bound.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("kind", ADVERSARIAL)
@pytest.mark.parametrize("K,N,M", [(64, 128, 333), (256, 1024, 97), (512, 256, 333)])
def test_tail_per_output_bound_on_adversarial_operands(kind, K, N, M):
    _check_per_output(TailCase(*_adversarial(kind, (M, K), (N, K), _gen("adv-tail", kind, K, N))), kind)


@pytest.mark.parametrize("kind", ADVERSARIAL)
@pytest.mark.parametrize("C,stride", sorted(CONV3_VARIANTS))
def test_conv3x3_per_output_bound_on_adversarial_operands(kind, C, stride):
    a, w = _adversarial(kind, (2, 9, 13, C), (C, 3, 3, C), _gen("adv-conv3", kind, C, stride))
    _check_per_output(Conv3Case(a, w, stride, CONV3_VARIANTS[(C, stride)]), kind)


@pytest.mark.parametrize("kind", ADVERSARIAL)
@pytest.mark.parametrize("C,N,stride", [(256, 128, 1), (256, 512, 2), (512, 1024, 2), (1024, 2048, 2)])
def test_conv1x1_strided_per_output_bound_on_adversarial_operands(kind, C, N, stride):
    a, w = _adversarial(kind, (2, 9, 13, C), (N, C), _gen("adv-strided", kind, C, N))
    _check_per_output(StridedCase(a, w, stride), kind)


@pytest.mark.parametrize("kind", ADVERSARIAL)
def test_stem_per_output_bound_on_adversarial_operands(kind):
    """The bound of a pooled output is the largest bound in its window (ReLU and max are 1-Lipschitz)."""
    a, w = _adversarial(kind, (2, 61, 83, 3), (64, 7, 7, 3), _gen("adv-stem", kind))
    _check_per_output(StemCase(a, w), kind)


# ---- item 5: the weight streams ---------------------------------------------------------------------------------------------------
def _wide(shape, g):
    """values at their own power of two 2^-100 .. 2^100, with zeros, a negative zero and fp32 denormals among them"""
    x = torch.randn(*shape, generator=g) * torch.pow(2.0, torch.randint(-100, 101, shape, generator=g).float())
    flat = x.view(-1)
    flat[::97] = 0.0
    flat[5] = -0.0
    flat[11::193] = flat[11::193].sign() * 1e-40
    return x


def _check_pieces(pieces, src, rne):
    """pieces == the host split of ``src`` bit for bit; hi + mid + lo == src; hi / mid / lo in this order"""
    want = (H.split3_rne if rne else H.split3_trunc)(src)
    for got, exp, name in zip(pieces, want, ("hi", "mid", "lo")):
        assert torch.equal(H._f32_bits(got), H._f32_bits(exp)), name
    hi, mid, lo = (p.double() for p in pieces)
    s, x = hi + mid + lo, src.double()
    full = x.abs() >= 2.0 ** -110                                  # three bf16 can hold all 24 bits (tests/test_split_arith_cpu.py)
    assert torch.equal(s[full], x[full])
    assert bool(((s - x).abs() <= torch.clamp(2.0 ** -24 * x.abs(), min=2.0 ** -133)).all())
    step = 2.0 ** -8 if rne else 2.0 ** -7                         # half a bf16 step by rounding, below one step by truncation
    assert bool((mid.abs() <= step * hi.abs()).all()) and bool((lo.abs() <= step * mid.abs()).all())


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("rows,K", [(1, 16), (37, 64), (100, 48), (256, 256), (333, 1024)])
def test_xs_split_streams_decode_to_the_host_split(weights, rows, K):
    """egtr_xs_split_f32, activation (truncation) and weight (nearest-even) mode, row counts that are not multiples of 32, a
    row-strided input, with and without ``pos`` (and pos alone): the stream decoded by the layout description equals the
    host split bit for bit."""
    from egtr_amd import ops
    g = _gen("xs", int(weights), rows, K)
    x_cpu = _wide((rows, K), g)
    x = x_cpu.to(DEV)
    assert ops.xs_bytes(rows, K) == ((rows + 31) // 32) * (K // 16) * 3 * 1024
    _check_pieces(H.xs_decode(ops.xs_split(x, weights=weights), rows, K), x_cpu, weights)
    wide = torch.zeros(rows, K + 64, device=DEV)
    wide[:, 32:32 + K] = x
    view = wide[:, 32:32 + K]
    assert view.stride(0) == K + 64 and view.data_ptr() % 16 == 0
    _check_pieces(H.xs_decode(ops.xs_split(view, weights=weights), rows, K), x_cpu, weights)
    pos_rows = max(1, rows // 3)
    pos_cpu = torch.randn(pos_rows, K, generator=g) * x_cpu[:pos_rows].abs()
    want_pos = x_cpu + pos_cpu[torch.arange(rows) % pos_rows]
    plain, with_pos = ops.xs_split(x, pos=pos_cpu.to(DEV), weights=weights)
    _check_pieces(H.xs_decode(plain, rows, K), x_cpu, weights)
    _check_pieces(H.xs_decode(with_pos, rows, K), want_pos, weights)
    none, only_pos = ops.xs_split(view, pos=pos_cpu.to(DEV), weights=weights, plain=False)
    assert none is None
    _check_pieces(H.xs_decode(only_pos, rows, K), want_pos, weights)


@pytest.mark.parametrize("C,stride", sorted(CONV3_VARIANTS))
def test_conv3x3_weight_streams_hold_the_split_weights_in_the_stated_order(C, stride):
    """ops.conv3x3_weights for every (C, stride, variant): the [N, 9 C] matrix in phases of CP channels, within a phase
    W[n][dy][dx][c'], every element the nearest-even split of its weight, hi / mid / lo in this order."""
    from egtr_amd import _lib, ops
    g = _gen("w3", C, stride)
    w_cpu = torch.randn(C, C, 3, 3, generator=g) * torch.pow(2.0, torch.randint(-12, 13, (C, 1, 1, 1), generator=g).float())
    w = w_cpu.to(DEV)
    for variant in CONV3_VARIANTS[(C, stride)]:
        cp = int(_lib.lib().egtr_conv3x3_phase_channels(C, C, stride, variant))
        assert cp > 0 and C % cp == 0
        pieces = H.xs_decode(ops.conv3x3_weights(w, stride, variant), C, 9 * C)
        back = [p.view(C, C // cp, 3, 3, cp).permute(0, 1, 4, 2, 3).reshape(C, C, 3, 3) for p in pieces]
        _check_pieces(back, w_cpu, True)
        # one element by its stated address
        n, c, dy, dx = C - 1, C - 3, 2, 1
        k = (c // cp) * 9 * cp + (dy * 3 + dx) * cp + c % cp
        assert float(pieces[0][n, k]) == float(H.split3_rne(w_cpu[n, c, dy, dx].view(1))[0])


def test_stem_weight_stream_holds_the_split_weights_and_exact_zero_padding():
    """ops.stem_weights: [64, 224] = per kernel row 8 taps x 4 channels; the padded tap and channel are zero in all three pieces."""
    from egtr_amd import ops
    g = _gen("wstem")
    w_cpu = torch.randn(64, 3, 7, 7, generator=g) * torch.pow(2.0, torch.randint(-12, 13, (64, 1, 1, 1), generator=g).float())
    pieces = [p.view(64, 7, 8, 4) for p in H.xs_decode(ops.stem_weights(w_cpu.to(DEV)), 64, 224)]
    _check_pieces([p[:, :, :7, :3].permute(0, 3, 1, 2).contiguous() for p in pieces], w_cpu, True)
    for p in pieces:
        assert int(H._f32_bits(p[:, :, 7, :]).abs().max()) == 0 and int(H._f32_bits(p[:, :, :, 3]).abs().max()) == 0
