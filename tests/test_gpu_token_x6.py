"""GPU (-m gpu): the ARITHMETIC of the token-sized split-bf16 kernels -- the forward product with its grouped and training entries
and the weight-gradient kernel (egtr_amd/csrc/gemm_split.hip), the FFN, the projection kernels and the encoder tail (egtr_amd/csrc/ffn_x6.hip),
layers 2 and 3 of the relation head (egtr_amd/csrc/rel_head.hip, rel_head_fwd_x6) -- and the weight streams they read, in the manner of
tests/test_gpu_backbone_x6.py: operands whose leading products cancel in adjacent k pairs (helpers.paired_operands and its
non-negative and truncation-truncation variants, checked on the host by tests/test_split_arith_cpu.py), every bar computed IN
the test from the fp64 restatement of the operands the kernel actually multiplies (E_model, E_loss, bar = sqrt(E_model E_loss),
E_loss >= 50 E_model and the torch fp32 composition under the bar asserted first), and teeth tests that remove one piece.

What is resolved by paired operands, and what only by code shared with a resolved stage:
  * gemm_split_bf16_f32 <64> and <128>: the main loop, through the single, grouped (``pos`` added on load) and ``ex`` entries
    (``row_keep``, ``colpart``).  The ``add1`` / ``add2`` / ``relu_ref`` epilogues add O(1) values behind the product and are
    covered by shared code only (tests/test_gpu_train_fused.py holds them to fp32 tolerances).
  * wgrad_split_bf16_f32 <false> and <true> (``x_pos`` on load, ``row_keep`` on g): both operands, pairs along m.
  * ffn_x6_kernel<false>: layer 1 (a 0 / 1 ``fc2`` returns a window of the hidden layer exactly) and layer 2 (identity ``fc1``
    hands the non-negative activations to the hidden layer exactly), each on its own.
  * proj_x6_kernel: as egtr_proj_ln_x6_f32 without LayerNorm and as egtr_proj_multi_x6_f32 with 1 and 6 weights.
  * ffn_x6_kernel<true> (the encoder tail): the output-projection stage, seen through LayerNorm1 -> FFN -> LayerNorm2.  The FFN
    stages of THIS instantiation cannot be isolated -- their input is LayerNorm1's result, computed in the kernel in fp32 -- and
    are covered only by the code they share with ffn_x6_kernel<false>.
  * rel_head_fwd_x6: layer 2 of both branches and layer 3 of the relation branch, the training entry (SAVE) once; layer 1 and
    the connectivity output are fp32 VALU work whose inputs are chosen so that they are exact or under the fp32 health check.
"""
import pytest
import torch
import torch.nn.functional as F

import helpers as H
from test_gpu_backbone_x6 import Case, _check_pieces, _check_six_terms, _check_teeth, _gen, _wide

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAMILIES = ["act", "wgt"]


def _linear(w, bias=None):
    """nn.Linear on the device with the given weight and a ZERO bias (or the given one)"""
    m = torch.nn.Linear(w.shape[1], w.shape[0]).to(DEV)
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.zero_() if bias is None else m.bias.copy_(bias)
    return m


def _mm(a, w):
    return a @ w.t()


# ---- 1. gemm_split_bf16_f32 ------------------------------------------------------------------------------------------------------
class GemmCase(Case):
    """entry: "single" (ops.linear_split_bf16), "tile" (the stream from ops.gemm_split_tile), "strided" (x a column block of a
    wider buffer), "grouped" (two problems in one launch, the second with ``pos`` = a_lo added on load to a_hi + a_mid, rows
    (row % pos_rows); pos_rows < M: the generator repeats its rows with that period), "ex" / "ex-keep" / "ex-colpart"
    (ops.linear_split_ex; ``row_keep`` zeroes rows, ``colpart`` returns the column sums of every 32-row block)."""
    op = staticmethod(_mm)

    def __init__(self, family, M, K, N, entry="single", pos_rows=None):
        g = _gen("gemm", family, M, K, N, entry, pos_rows or 0)
        rows = pos_rows or M
        a, w = H.paired_operands(family, (rows, K), (N, K), g)
        self.a, self.w = a.repeat(M // rows, 1).to(DEV), w.to(DEV)
        self.M, self.K, self.N, self.entry, self.pos_rows = M, K, N, entry, rows
        self.name = f"gemm_split {entry} M={M} K={K} N={N}" + (f" pos_rows={rows}" if entry == "grouped" else "")
        if entry == "ex-keep":
            self.keep = (torch.rand(M, generator=g) < 0.7).to(DEV)
            self.post = lambda t: t * self.keep.to(t.dtype)[:, None]
        if entry == "ex-colpart":
            pad = (-M) % 32
            self.post = lambda t: F.pad(t, (0, 0, 0, pad)).view(-1, 32, t.shape[1]).sum(1)

    def runs(self, a, w):
        from egtr_amd import ops
        M, K, N, e = self.M, self.K, self.N, self.entry
        wt = ops.gemm_split_tile(w) if e == "tile" else ops.gemm_split_weights(w)
        zero = torch.zeros(N, device=DEV)
        if e in ("single", "tile"):
            return [(e, ops.linear_split_bf16(a, wt, zero if e == "tile" else None, N))]
        if e == "strided":
            wide = torch.full((M, K + 8), 3.0, device=DEV)
            wide[:, :K] = a
            view = wide[:, :K]
            assert view.stride(0) == K + 8
            return [(e, ops.linear_split_bf16(view, wt, None, N))]
        if e == "grouped":
            x, lo = (t.to(DEV) for t in H.add_on_load(a.cpu()))
            assert float(lo.abs().max()) > 0
            pos = lo[:self.pos_rows].contiguous()
            assert torch.equal(x + pos.repeat(M // self.pos_rows, 1), a)
            y0, y1 = ops.linear_split_bf16_grouped([dict(x=a, wt=wt, N=N, b=zero), dict(x=x, wt=wt, N=N, pos=pos)])
            return [("plain", y0), ("pos on load", y1)]
        item = dict(x=a, wt=wt, N=N, b=zero)
        if e == "ex-keep":
            item["row_keep"] = self.keep.to(torch.uint8)
        if e == "ex-colpart":
            item["colpart"] = torch.full(((M + 31) // 32, N), float("nan"), device=DEV)
        (y,) = ops.linear_split_ex([item], M, K)
        return [(e, item["colpart"] if e == "ex-colpart" else y)]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("M", [37, 200])
@pytest.mark.parametrize("K", [32, 256, 1024])
@pytest.mark.parametrize("N", [128, 384])
def test_gemm_split_64_keeps_all_six_terms(family, M, K, N):
    """gemm_split_bf16_f32<64>: a partial row tile and several, one K stage and many, one and three n blocks"""
    _check_six_terms(GemmCase(family, M, K, N), family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("entry", ["tile", "strided"])
def test_gemm_split_stream_from_the_tiling_kernel_and_row_strided_input(family, entry):
    _check_six_terms(GemmCase(family, 200, 256, 384, entry), family)


@pytest.mark.parametrize("family", FAMILIES)
def test_gemm_split_128_keeps_all_six_terms(family):
    """gemm_split_bf16_f32<128>: egtr_amd/csrc/gemm_split.hip::launch_grouped takes it when sum (N / 128) ceil(M / 128) >= 480; here
    (2048 / 128) * ceil(3905 / 128) = 16 * 31 = 496, the last row tile partial (3905 = 30 * 128 + 65)."""
    M, K, N = 3905, 64, 2048
    assert (N // 128) * ((M + 127) // 128) >= 480
    _check_six_terms(GemmCase(family, M, K, N), family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("pos_rows", [200, 100])
def test_gemm_split_grouped_entry_with_pos_added_on_load(family, pos_rows):
    """egtr_linear_split_bf16_grouped_pos_f32, two problems in one launch; the second multiplies fl32(x + pos) == a bit for bit
    (helpers.add_on_load), pos_rows = M and M / 2."""
    _check_six_terms(GemmCase(family, 200, 256, 128, "grouped", pos_rows), family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("entry", ["ex", "ex-keep", "ex-colpart"])
def test_gemm_split_ex_entry_keeps_all_six_terms(family, entry):
    """egtr_linear_split_bf16_ex_f32 with a zero bias: plain, ``row_keep`` (post = the row mask) and ``colpart`` (post = the
    32-row block column sums; the kernel's fp32 summation is part of what is measured, the fp32 route sums in fp32 too)."""
    _check_six_terms(GemmCase(family, 200, 256, 128, entry), family)


@pytest.mark.parametrize("family", FAMILIES)
def test_gemm_split_bar_is_exceeded_when_one_piece_is_removed(family):
    _check_teeth(GemmCase(family, 200, 256, 384), family)


# ---- 2. wgrad_split_bf16_f32 -----------------------------------------------------------------------------------------------------
class WgradCase(Case):
    """a = g [M, N], w = x [M, K], both split by truncation, pairs = adjacent rows m.  An odd M (the issue's 33 and 777) leaves
    one row without a partner, whose leading product nothing cancels: its g row is ZERO (x keeps random values), so the ragged
    last stage still runs.  ``ex``: x arrives as x_hi + x_mid with x_pos = x_lo (pos_rows = M), and ``row_keep`` masks whole
    pairs of g rows, which hold junk in the operand the kernel is given."""
    a_split = w_split = staticmethod(H.split3_trunc)

    def __init__(self, family, M, N, K, ex=False):
        gen = _gen("wgrad", family, M, N, K, int(ex))
        Me = M - M % 2
        gt, xt = H.paired_operands_trunc(family, (N, Me), (K, Me), gen)
        g, x = torch.zeros(M, N), torch.randn(M, K, generator=gen)
        g[:Me], x[:Me] = gt.t(), xt.t()
        self.M, self.ex, self.name = M, ex, f"wgrad{' ex' if ex else ''} M={M} N={N} K={K}"
        if ex:
            keep = (torch.rand((M + 1) // 2, generator=gen) < 0.7).repeat_interleave(2)[:M]
            self.keep = keep.to(DEV)
            g = g * keep[:, None]
        self.a, self.w = g.to(DEV), x.to(DEV)

    @staticmethod
    def op(g, x):
        return g.t() @ x

    def runs(self, g, x):
        from egtr_amd import ops
        if not self.ex:
            return [("", ops.linear_split_bf16_wgrad(g, x))]
        xx, pos = (t.to(DEV) for t in H.add_on_load(x.cpu()))
        junk = torch.where(self.keep[:, None], g, torch.full_like(g, 3.0))
        return [("x_pos, row_keep", ops._wgrad_ex(junk, xx, x_pos=pos, row_keep=self.keep.to(torch.uint8)))]


def _wgrad_plan(M, N, K):
    """(chunks, rows per chunk, stages of the last chunk, rows of its last stage): egtr_amd/csrc/gemm_split.hip::wgrad_plan
    restated -- split-K chunks = min(ceil(512 / tiles), ceil(M / 32)) with tiles = (N / 128)(K / 128), rows per chunk rounded
    up to the 32-row stage; the chunk count is checked against the workspace size the library reports."""
    from egtr_amd import _lib
    tiles = (N // 128) * (K // 128)
    chunks = min(max(1, -(-512 // tiles)), -(-M // 32))
    rpc = -(-(-(-M // chunks)) // 32) * 32
    chunks = -(-M // rpc)
    assert int(_lib.lib().egtr_linear_split_bf16_wgrad_workspace_floats(M, N, K, 6)) == chunks * N * K
    last = M - (chunks - 1) * rpc
    return chunks, rpc, -(-last // 32), (last - 1) % 32 + 1


# (M, N, K) -> (chunks, rows per chunk, stages of the last chunk, rows of its last stage)
WGRAD_SHAPES = {(33, 128, 128): (2, 32, 1, 1),          # a chunk of one row: the ragged stage
                (777, 128, 128): (25, 32, 1, 9),        # many one-stage chunks
                (4100, 128, 128): (129, 32, 1, 4),      # the ceil(M / 32) limit on the chunk count
                (33, 256, 128): (2, 32, 1, 1), (777, 256, 128): (25, 32, 1, 9), (4100, 256, 128): (129, 32, 1, 4),
                (4134, 256, 256): (65, 64, 2, 6),       # two stages per chunk (the loop over s + 1), the last one ragged
                (16502, 128, 128): (258, 64, 2, 22)}    # the same at the 512-chunk limit of a single tile


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("M,N,K", sorted(WGRAD_SHAPES))
def test_wgrad_keeps_all_six_terms(family, M, N, K):
    """wgrad_split_bf16_f32<false>: a ragged chunk, many one-stage chunks, wgrad_plan's ceil(M / 32) chunk limit, and chunks of
    two stages with a ragged last stage.  With N, K <= 256 the plan gives 32-row chunks (one stage) up to M = 32 * 512 / tiles,
    so the multi-stage shapes are (256, 256) at M = 4134 and (128, 128) at M = 16502; the plan of every shape is asserted."""
    assert _wgrad_plan(M, N, K) == WGRAD_SHAPES[(M, N, K)]
    _check_six_terms(WgradCase(family, M, N, K), family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("M,N,K", [(33, 128, 128), (777, 128, 128), (4134, 256, 256)])
def test_wgrad_ex_keeps_all_six_terms(family, M, N, K):
    """wgrad_split_bf16_f32<true>: one-stage chunks and two-stage chunks with a ragged last stage"""
    assert _wgrad_plan(M, N, K) == WGRAD_SHAPES[(M, N, K)]
    _check_six_terms(WgradCase(family, M, N, K, ex=True), family)


@pytest.mark.parametrize("family", FAMILIES)
def test_wgrad_bar_is_exceeded_when_one_piece_is_removed(family):
    """"act": g - g_lo, "wgt": x - x_lo; two-stage chunks"""
    assert _wgrad_plan(4134, 256, 256)[1:3] == (64, 2)
    _check_teeth(WgradCase(family, 4134, 256, 256), family)


# ---- 3. ffn_x6_kernel<false> -----------------------------------------------------------------------------------------------------
class FfnLayer1Case(Case):
    """fc1 paired; fc2 a 0 / 1 selector of a window of min(F, 256) hidden units (F / 256 launches), zero biases; post = relu"""
    op = staticmethod(_mm)
    post = staticmethod(torch.relu)

    def __init__(self, family, M, Fdim):
        a, w = H.paired_operands(family, (M, 256), (Fdim, 256), _gen("ffn1", family, M, Fdim))
        self.a, self.w, self.F, self.name = a.to(DEV), w.to(DEV), Fdim, f"ffn layer 1 M={M} F={Fdim}"

    def runs(self, a, w):
        from egtr_amd import ops
        fc1, width, outs = _linear(w), min(self.F, 256), []
        for lo in range(0, self.F, width):
            sel = torch.zeros(256, self.F, device=DEV)
            sel[torch.arange(width), lo + torch.arange(width)] = 1.0
            outs.append(ops.ffn_fused(a, fc1, _linear(sel))[:, :width])
        return [("", torch.cat(outs, 1))]


class FfnLayer2Case(Case):
    """fc1 = F / 256 stacked identities, so the hidden layer is the non-negative x repeated F / 256 times, exactly; fc2 paired
    over all F columns.  ``a`` is the hidden layer [M, F]; the kernel gets its first 256 columns."""
    op = staticmethod(_mm)

    def __init__(self, family, M, Fdim):
        a, w = H.paired_operands(family, (M, Fdim), (256, Fdim), _gen("ffn2", family, M, Fdim), nonneg=True)
        self.a, self.w, self.F = a[:, :256].repeat(1, Fdim // 256).to(DEV), w.to(DEV), Fdim
        self.name = f"ffn layer 2 M={M} F={Fdim}"

    def runs(self, a, w):
        from egtr_amd import ops
        assert torch.equal(a, a[:, :256].repeat(1, self.F // 256)) and bool((a >= 0).all())
        eye = torch.eye(256, device=DEV).repeat(self.F // 256, 1)
        return [("", ops.ffn_fused(a[:, :256].contiguous(), _linear(eye), _linear(w)))]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("M", [37, 200])
@pytest.mark.parametrize("Fdim", [64, 1024])
def test_ffn_layer1_keeps_all_six_terms(family, M, Fdim):
    _check_six_terms(FfnLayer1Case(family, M, Fdim), family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("M", [37, 200])
@pytest.mark.parametrize("Fdim", [256, 1024])
def test_ffn_layer2_keeps_all_six_terms(family, M, Fdim):
    _check_six_terms(FfnLayer2Case(family, M, Fdim), family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("layer", [FfnLayer1Case, FfnLayer2Case])
def test_ffn_bar_is_exceeded_when_one_piece_is_removed(family, layer):
    _check_teeth(layer(family, 200, 1024), family)


# ---- 4., 5. proj_x6_kernel -------------------------------------------------------------------------------------------------------
class ProjCase(Case):
    """num_weights = 0: ops.proj_ln_fused(x, lin) without LayerNorm (zero bias); else ops.proj_multi_fused with that many
    stacked 256 x 256 weights, with a zero bias or none."""

    def __init__(self, family, M, nw=0, bias=False):
        a, w = H.paired_operands(family, (M, 256), (max(nw, 1) * 256, 256), _gen("proj", family, M, nw))
        self.a, self.w, self.nw, self.bias = a.to(DEV), w.to(DEV), nw, bias
        self.name = f"proj_ln M={M}" if nw == 0 else f"proj_multi M={M} num_weights={nw} bias={bias}"

    def op(self, a, w):
        y = a @ w.t()
        return y if self.nw == 0 else y.view(a.shape[0], self.nw, 256).transpose(0, 1)

    def runs(self, a, w):
        from egtr_amd import ops
        if self.nw == 0:
            return [("", ops.proj_ln_fused(a, _linear(w)))]
        b = torch.zeros(self.nw * 256, device=DEV) if self.bias else None
        return [("", ops.proj_multi_fused(a, ops.xs_split(w.contiguous(), weights=True), self.nw, b))]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("M", [37, 200])
def test_proj_ln_keeps_all_six_terms(family, M):
    _check_six_terms(ProjCase(family, M), family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("M", [65, 200])
@pytest.mark.parametrize("nw", [1, 6])
@pytest.mark.parametrize("bias", [False, True])
def test_proj_multi_keeps_all_six_terms(family, M, nw, bias):
    _check_six_terms(ProjCase(family, M, nw, bias), family)


@pytest.mark.parametrize("family", FAMILIES)
def test_proj_ln_bar_is_exceeded_when_one_piece_is_removed(family):
    _check_teeth(ProjCase(family, 200), family)


@pytest.mark.parametrize("family", FAMILIES)
def test_proj_multi_bar_is_exceeded_when_one_piece_is_removed(family):
    _check_teeth(ProjCase(family, 200, 6, True), family)


# ---- 6. ffn_x6_kernel<true> ------------------------------------------------------------------------------------------------------
class EncoderTailCase(Case):
    """The output projection is paired; hidden = 0 and a zero out_proj.bias, so LayerNorm1 sees the projected rows alone.  The
    context is scaled by 2^12: the paired rows then have variance ~ 10, far above LayerNorm's eps = 1e-5, which would otherwise
    swamp a result that lives at 2^-9.  post = LayerNorm1 -> FFN -> LayerNorm2 with ordinary random parameters, in the dtype of
    its argument (fp64 for every restatement).  The FFN stages of this instantiation cannot be isolated: their input is computed
    in the kernel in fp32."""
    op = staticmethod(_mm)

    def __init__(self, family, M, Fdim=1024):
        g = _gen("tail", family, M, Fdim)
        a, w = H.paired_operands(family, (M, 256), (256, 256), g)
        self.a, self.w, self.name = (a * 2.0 ** 12).to(DEV), w.to(DEV), f"encoder tail M={M} F={Fdim}"
        r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(DEV)  # noqa: E731
        self.fc1, self.fc2 = _linear(r(Fdim, 256, sc=1 / 16), r(Fdim, sc=0.1)), _linear(r(256, Fdim, sc=1 / 32), r(256, sc=0.1))
        self.ln1, self.ln2 = torch.nn.LayerNorm(256).to(DEV), torch.nn.LayerNorm(256).to(DEV)
        with torch.no_grad():
            for ln in (self.ln1, self.ln2):
                ln.weight.copy_(1 + r(256, sc=0.1))
                ln.bias.copy_(r(256, sc=0.1))

    def post(self, t):
        c = lambda p: p.detach().to(t.dtype)  # noqa: E731
        ln = lambda x, m: F.layer_norm(x, (256,), c(m.weight), c(m.bias), m.eps)  # noqa: E731
        y1 = ln(t, self.ln1)
        return ln(y1 + F.linear(torch.relu(F.linear(y1, c(self.fc1.weight), c(self.fc1.bias))), c(self.fc2.weight),
                                c(self.fc2.bias)), self.ln2)

    def runs(self, a, w):
        from egtr_amd import ops
        return [("", ops.encoder_tail_fused(a, torch.zeros_like(a), _linear(w), self.ln1, self.fc1, self.fc2, self.ln2))]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("M", [37, 200])
def test_encoder_tail_projection_keeps_all_six_terms(family, M):
    _check_six_terms(EncoderTailCase(family, M), family)


@pytest.mark.parametrize("family", FAMILIES)
def test_encoder_tail_bar_is_exceeded_when_one_piece_is_removed(family):
    _check_teeth(EncoderTailCase(family, 200), family)


# ---- 7. rel_head_fwd_x6 ----------------------------------------------------------------------------------------------------------
class RelHeadCase(Case):
    """One slot per query (T = 1; the training entry needs T = 4: slots 1 .. 3 hold zeros), gate_q = gate_k = 40 so that every
    gate is 1.0 in fp32, uk = 0, b1 = 0: the layer-2 activations of pair (i, j) are uq[i] exactly, non-negative by construction.
    stage "l2rel": w2r paired, w3r a 0 / 1 selector of 64 of the 256 units (four launches), post = relu;  "l3rel": w2r = I,
    w3r [R, 256] paired;  "l2conn": w2c paired, w3c = random signs +-1, post = relu then the signed row sum (an fp32 VALU dot in
    the kernel).  CHANGED from an all-ones w3c: the plain sum of 256 non-negative units adds the signal coherently (x 256) and
    a lost term's error like a random walk (x 16), while the "wgt" family's six-term error is coherent too, so E_loss / E_model
    fell to 14-23 (restated on the host); with signs every part grows like a random walk and the ratio is that of the units
    themselves, 135-165.  Products with +-1 are exact.  Every bias is zero.  ``a`` is [B, N, 256]; the outputs repeat over j."""

    def __init__(self, family, stage, B, N, R=64, train=False):
        rows = R if stage == "l3rel" else 256
        a, w = H.paired_operands(family, (B, N, 256), (rows, 256), _gen("rel", family, stage, B, N, R), nonneg=True)
        self.a, self.w, self.stage, self.B, self.N, self.R, self.train = a.to(DEV), w.to(DEV), stage, B, N, R, train
        self.name = f"rel_head {stage}{' train' if train else ''} B={B} N={N} R={R}"
        self.sign = torch.where(torch.rand(256, generator=_gen("sign", B, N)) < 0.5, -1.0, 1.0).to(DEV)
        if stage != "l3rel":
            self.post = torch.relu if stage == "l2rel" else (lambda t: (torch.relu(t) * self.sign.to(t.dtype)).sum(-1, keepdim=True))

    def op(self, a, w):
        y = a @ w.t()
        return y[:, :, None, :].expand(self.B, self.N, self.N, y.shape[-1])

    def _launch(self, a, w2r, w3r, w2c, w3c):
        from egtr_amd import ops
        B, N, R, T = self.B, self.N, w3r.shape[0], 4 if self.train else 1
        z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
        uq = z(B, N, T, 512)
        uq[:, :, 0, 256 * (self.stage == "l2conn"):][..., :256] = a
        gate = torch.full((B, N, T), 40.0, device=DEV)
        if self.train:
            assert ops.REL_HEAD_TRAIN_X6 and ops.GEMM_SPLIT_BF16
            rel, conn, gm = ops.RelationHeadFunction.apply(gate, gate, uq.requires_grad_(), z(B, N, T, 512), z(512), w2r, z(256),
                                                           w3r, z(R), w2c, z(256), w3c, z(1), None, None, True)
            rel, conn = rel.detach(), conn.detach()
        else:
            w2xr, w3xr, w2xc = ops.rel_head_split_weights(w2r, w3r, w2c)
            rel, conn, gm = ops.relation_head_split_bf16(gate, gate, uq, z(B, N, T, 512), z(512), w2xr, z(256), w3xr, z(R), w2xc,
                                                         z(256), w3c, z(1), R, want_gate_mean=True)
        # every gate is 1 (test_relation_head_gates_are_exactly_one shows it bit for bit): the mean is then the sum over
        # workgroups of fl32(pairs of the workgroup / all pairs), each quotient and each addition rounded once
        blocks = B * ((N + 7) // 8) * ((N + 3) // 4)
        assert float((gm - 1).abs().max()) <= (2 * blocks) * 2.0 ** -24, gm
        return rel, conn, gm

    def runs(self, a, w):
        z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
        eye, w3c = torch.eye(256, device=DEV), self.sign.view(1, 256).contiguous()
        if self.stage == "l3rel":
            return [("", self._launch(a, eye, w, z(256, 256), w3c)[0])]
        if self.stage == "l2conn":
            return [("", self._launch(a, z(256, 256), z(self.R, 256), w, w3c)[1])]
        outs = []
        for lo in range(0, 256, 64):
            sel = z(64, 256)
            sel[torch.arange(64), lo + torch.arange(64)] = 1.0
            outs.append(self._launch(a, w, sel, z(256, 256), w3c)[0])
        return [("", torch.cat(outs, -1))]


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("B,N", [(1, 8), (2, 33)])
def test_relation_head_gates_are_exactly_one(B, N, train):
    """What the cases below rest on, shown directly: with gate logits 40 + 40, uk = 0, b1 = 0, w2r = I and a 0 / 1 w3r the
    relation output of pair (i, j) is uq[i] on the selected units BIT FOR BIT (a gate of 1 - 2^-24 would change almost every
    value; identity and selector products are exact, tests/test_split_arith_cpu.py), in the inference and the training entry.
    Where the pair count of every workgroup (8 x 4 pairs) and the total are powers of two (B = 1, N = 8) the quotients of the
    gate mean are exact and the mean is exactly 1."""
    case = RelHeadCase("wgt", "l3rel", B, N, 64, train=train)
    eye = torch.eye(256, device=DEV)
    for lo in range(0, 256, 64):
        sel, none = eye[lo:lo + 64].contiguous(), torch.zeros(256, 256, device=DEV)
        rel, _, gm = case._launch(case.a, eye, sel, none, case.sign.view(1, 256))
        want = case.a[:, :, None, lo:lo + 64].expand(B, N, N, 64)
        assert torch.equal(H._f32_bits(rel), H._f32_bits(want))
        if (B, N) == (1, 8):
            assert bool((gm == 1).all()), gm


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B,N", [(1, 7), (2, 33)])
@pytest.mark.parametrize("stage", ["l2rel", "l2conn"])
def test_relation_head_layer2_keeps_all_six_terms(family, B, N, stage):
    _check_six_terms(RelHeadCase(family, stage, B, N), family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B,N", [(1, 33), (2, 7)])
@pytest.mark.parametrize("R", [7, 50, 64])
def test_relation_head_layer3_keeps_all_six_terms(family, B, N, R):
    _check_six_terms(RelHeadCase(family, "l3rel", B, N, R), family)


@pytest.mark.parametrize("family", FAMILIES)
def test_relation_head_training_entry_keeps_all_six_terms(family):
    """egtr_rel_head_forward_bf16x6_save_f32 through ops.RelationHeadFunction (T = 4, gradients required)"""
    _check_six_terms(RelHeadCase(family, "l3rel", 2, 33, 50, train=True), family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("stage", ["l2rel", "l3rel", "l2conn"])
def test_relation_head_bar_is_exceeded_when_one_piece_is_removed(family, stage):
    _check_teeth(RelHeadCase(family, stage, 2, 33, 50 if stage == "l3rel" else 64), family)


# ---- the weight streams: bit for bit ---------------------------------------------------------------------------------------------
def _gemm_pieces(stream, N, K):
    """[N/128][K/32][3 pieces][128][32] bf16 -> the three [N, K] pieces"""
    assert stream.dtype == torch.bfloat16 and tuple(stream.shape) == (N // 128, K // 32, 3, 128, 32)
    return [stream[:, :, p].permute(0, 2, 1, 3).reshape(N, K).float().cpu() for p in range(3)]


def test_gemm_split_weight_streams_decode_to_the_host_split():
    """ops.gemm_split_weights, ops.gemm_split_tile (plain and transposed), ops.gemm_split_tile_pair and
    ops.gemm_split_tile_pairs with a concatenated pair, on values across 2^+-100 with zeros, -0 and denormals"""
    from egtr_amd import ops
    g = _gen("gemm-streams")
    w_cpu, wb_cpu = _wide((256, 384), g), _wide((128, 384), g)
    w, wb = w_cpu.to(DEV), wb_cpu.to(DEV)
    _check_pieces(_gemm_pieces(ops.gemm_split_weights(w), 256, 384), w_cpu, True)
    _check_pieces(_gemm_pieces(ops.gemm_split_tile(w), 256, 384), w_cpu, True)
    _check_pieces(_gemm_pieces(ops.gemm_split_tile(w, transposed=True), 384, 256), w_cpu.t().contiguous(), True)
    wide = torch.zeros(256, 384 + 64, device=DEV)
    wide[:, 32:32 + 384] = w
    _check_pieces(_gemm_pieces(ops.gemm_split_tile(wide[:, 32:32 + 384]), 256, 384), w_cpu, True)
    fwd, bwd = ops.gemm_split_tile_pair(w)
    _check_pieces(_gemm_pieces(fwd, 256, 384), w_cpu, True)
    _check_pieces(_gemm_pieces(bwd, 384, 256), w_cpu.t().contiguous(), True)
    cat = torch.cat([w_cpu, wb_cpu], 0)
    (f1, b1), (f2, b2) = ops.gemm_split_tile_pairs([(w, wb), wb])
    _check_pieces(_gemm_pieces(f1, 384, 384), cat, True)
    _check_pieces(_gemm_pieces(b1, 384, 384), cat.t().contiguous(), True)
    _check_pieces(_gemm_pieces(f2, 128, 384), wb_cpu, True)
    _check_pieces(_gemm_pieces(b2, 384, 128), wb_cpu.t().contiguous(), True)


def _rel_head_pieces(w2x, w3x, OT):
    """egtr_amd/csrc/rel_head.hip: w2x [8 nt][16 t][3 piece][2 hf][32 pi][8 e] = piece of W2[32 nt + pi][16 t + 8 hf + e];
    w3x [8 nt][2 kb][OT][3 piece][2 hf][32 pi][8 e] = piece of W3[32 ot + pi][32 nt + 16 kb + (e & 3) + 8 (e >> 2) + 4 hf]"""
    assert tuple(w2x.shape) == (8, 16, 3, 2, 32, 8) and tuple(w3x.shape) == (8, 2, OT, 3, 2, 32, 8)
    w2 = [w2x[:, :, p].permute(0, 3, 1, 2, 4).reshape(256, 256).float().cpu() for p in range(3)]
    ix = torch.arange
    nt, kb, ot = ix(8).view(8, 1, 1, 1, 1, 1), ix(2).view(1, 2, 1, 1, 1, 1), ix(OT).view(1, 1, OT, 1, 1, 1)
    hf, pi, e = ix(2).view(1, 1, 1, 2, 1, 1), ix(32).view(1, 1, 1, 1, 32, 1), ix(8).view(1, 1, 1, 1, 1, 8)
    row = (32 * ot + pi).expand(8, 2, OT, 2, 32, 8)
    col = (32 * nt + 16 * kb + (e & 3) + 8 * (e >> 2) + 4 * hf).expand(8, 2, OT, 2, 32, 8)
    w3 = []
    for p in range(3):
        m = torch.full((32 * OT, 256), float("nan"))
        m[row, col] = w3x[:, :, :, p].float().cpu()
        w3.append(m)
    return w2, w3


@pytest.mark.parametrize("R", [7, 50, 64])
@pytest.mark.parametrize("builder", ["rel_head_split_weights", "rel_head_streams"])
def test_relation_head_weight_streams_decode_to_the_host_split(builder, R):
    from egtr_amd import ops
    g = _gen("rel-streams", R)
    w2r, w3r, w2c = _wide((256, 256), g), _wide((R, 256), g), _wide((256, 256), g)
    w2xr, w3x, w2xc = getattr(ops, builder)(w2r.to(DEV), w3r.to(DEV), w2c.to(DEV))
    OT = 1 if R <= 32 else 2
    p2r, p3 = _rel_head_pieces(w2xr, w3x, OT)
    p2c, _ = _rel_head_pieces(w2xc, w3x, OT)
    _check_pieces(p2r, w2r, True)
    _check_pieces(p2c, w2c, True)
    _check_pieces([m[:R].contiguous() for m in p3], w3r, True)
    if R < 32 * OT:                                                        # the padding rows: zero in every piece
        assert all(int(H._f32_bits(m[R:]).max()) == 0 for m in p3)
