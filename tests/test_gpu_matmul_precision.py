"""GPU (-m gpu): the opt-in bf16 matmul precision of the training token GEMMs (egtr_amd.ops.set_matmul_precision, DESIGN.md
4.12b): the one-term kernels gemm_bf16r_f32 / wgrad_bf16r_f32 and the one-piece tiling launches (egtr_amd/csrc/gemm_split.hip)
through the ``terms=1`` bindings, and the three autograd Functions under the mode.

Products are held to the DERIVED bar of tests/test_matmul_precision_cpu.py: against the float64 product of the RNE-rounded
operands, 2 K 2^-24 sum |a_r w_r| per element (+ one fp32 rounding per O(1) epilogue addend); each product test first asserts
on the host that this bar separates the RNE product from truncated operands, unrounded operands (a switch that does nothing)
and a dropped k-step on the very inputs it uses.  A layer chains products through LayerNorm and MSDA, where a last-bit
difference upstream can flip a rounding downstream: the layer tests MEASURE instead (see there)."""
import pytest
import torch
import torch.nn.functional as F

from test_matmul_precision_cpu import (FORWARD_SHAPES, U, WGRAD_SHAPES, assert_teeth, operand, product_ref, rne)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _check(got, ref, bar, name):
    err = (got.detach().double().cpu() - ref).abs()
    worst = (err / bar.clamp_min(1e-300)).max().item()
    print(f"{name}: worst error / bar = {worst:.3g}, largest error {err.max().item():.3g}")
    assert bool((err <= bar).all()), (name, worst)


def _stream(w, how):
    from egtr_amd import ops
    host = ops.gemm_split_weights(w, terms=1).to(DEV)
    if how == "host":
        return host
    tiled = ops.gemm_split_tile(w.to(DEV), terms=1)
    assert tiled.shape == host.shape and torch.equal(_bits(tiled), _bits(host)), "tiling launch != host restatement"
    return tiled


# ---- forward kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N", FORWARD_SHAPES)
def test_forward_single_entry_vs_float64_of_the_rounded_operands(M, K, N):
    """gemm_bf16r_f32<64, .>: a partial row tile and several; K = 32 (one stage of the depth-32 form), 64 (one deep stage), 256 and
    1024 (many); one and three n blocks; the stream from the tiling launch and from the host restatement (bit-equal streams,
    then bit-equal results)."""
    from egtr_amd import ops
    a, w = operand((M, K), 11), operand((N, K), 12, scale=1.0 / 16)
    assert_teeth(a, w)
    ref, bar = product_ref(a, w)
    y_host = ops.linear_split_bf16(a.to(DEV), _stream(w, "host"), None, N, terms=1)
    y_tile = ops.linear_split_bf16(a.to(DEV), _stream(w, "tile"), None, N, terms=1)
    _check(y_host, ref, bar, f"forward {M}x{K}->{N}")
    assert torch.equal(y_host, y_tile)


def test_forward_row_strided_input_and_bias_relu():
    """x a column block of a wider buffer (row stride K + 8); bias and ReLU in the epilogue"""
    from egtr_amd import ops
    M, K, N = 200, 256, 384
    a, w = operand((M, K), 21), operand((N, K), 22, scale=1.0 / 16)
    assert_teeth(a, w)
    ref, bar = product_ref(a, w)
    wide = torch.full((M, K + 8), 3.0, device=DEV)
    wide[:, :K] = a.to(DEV)
    view = wide[:, :K]
    assert view.stride(0) == K + 8
    wt = _stream(w, "tile")
    _check(ops.linear_split_bf16(view, wt, None, N, terms=1), ref, bar, "row-strided")
    b = -ref.mean(0).float()                  # centres the columns: about half of the outputs are cut by the ReLU
    v = ref + b.double()
    got = ops.linear_split_bf16(a.to(DEV), wt, b.to(DEV), N, relu=True, terms=1)
    assert 0.2 < (v > 0).double().mean().item() < 0.8
    _check(got, v.clamp_min(0), bar + U * (v.abs() + bar), "bias + relu")


def test_forward_taller_row_tile():
    """gemm_bf16r_f32<128, .>: launch_grouped takes 128-row tiles when sum (N / 128) ceil(M / 128) >= 480, as for the six-term
    kernel; (2048 / 128) * ceil(3905 / 128) = 496, the last row tile partial.  K = 64: the deep stage; K = 96: the depth-32 form."""
    from egtr_amd import ops
    for K in (64, 96):
        M, N = 3905, 2048
        assert (N // 128) * ((M + 127) // 128) >= 480
        a, w = operand((M, K), 31), operand((N, K), 32, scale=1.0 / 16)
        assert_teeth(a, w)
        ref, bar = product_ref(a, w)
        _check(ops.linear_split_bf16(a.to(DEV), _stream(w, "tile"), None, N, terms=1), ref, bar, f"128-row tiles K={K}")


@pytest.mark.parametrize("pos_rows", [200, 100])
def test_grouped_launch_with_pos_added_on_load(pos_rows):
    """two problems in one launch; the second multiplies RNE(fl32(x + pos)): x + pos == a exactly in fp32, while neither x nor
    pos is a bf16 value, so rounding before the add gives another product"""
    from egtr_amd import ops
    M, K, N = 200, 256, 128
    a, w = operand((M, K), 41), operand((N, K), 42, scale=1.0 / 16)
    a2, w2 = operand((M, K), 43), operand((384, K), 44, scale=1.0 / 16)
    g = torch.Generator().manual_seed(45)
    pos = (torch.randint(1, 2 ** 15, (pos_rows, K), generator=g).double() / 2 ** 18).float()      # multiples of 2^-18 below 1/8
    x = a2 - pos.repeat(M // pos_rows, 1)
    assert torch.equal((x + pos.repeat(M // pos_rows, 1)), a2)
    assert not torch.equal(rne(x) + rne(pos).repeat(M // pos_rows, 1), rne(a2))
    assert_teeth(a, w)
    assert_teeth(a2, w2)
    y0, y1 = ops.linear_split_ex([dict(x=a.to(DEV), wt=_stream(w, "tile"), N=N),
                                  dict(x=x.to(DEV), wt=_stream(w2, "tile"), N=384, pos=pos.to(DEV))], M, K, terms=1)
    _check(y0, *product_ref(a, w), "grouped, plain")
    _check(y1, *product_ref(a2, w2), f"grouped, pos_rows={pos_rows}")


@pytest.mark.parametrize("option", ["row_keep", "relu", "relu_ref", "add1+add2", "colpart"])
def test_ex_entry_options_vs_float64_of_the_rounded_operands(option):
    from egtr_amd import ops
    M, K, N = 203, 256, 128                  # not a multiple of 32: the last colpart block is partial
    a, w = operand((M, K), 51), operand((N, K), 52, scale=1.0 / 16)
    assert_teeth(a, w)
    ref, bar = product_ref(a, w)
    g = torch.Generator().manual_seed(53)
    item = dict(x=a.to(DEV), wt=_stream(w, "tile"), N=N)
    want = ref
    if option == "row_keep":
        keep = torch.rand(M, generator=g) < 0.7
        item["row_keep"] = keep.to(torch.uint8).to(DEV)
        want = ref * keep.double()[:, None]
    elif option == "relu":
        b = -ref.mean(0).float()
        item.update(b=b.to(DEV), relu=True)
        v = ref + b.double()
        want, bar = v.clamp_min(0), bar + U * (v.abs() + bar)
    elif option == "relu_ref":
        r = torch.randn(M, N, generator=g)
        item["relu_ref"] = r.to(DEV)
        want = torch.where(r > 0, ref, torch.zeros_like(ref))
    elif option == "add1+add2":
        a1, a2 = torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
        out = a1.to(DEV).clone()             # add1 aliases the output
        item.update(add1=out, add2=a2.to(DEV), out=out)
        v1 = ref + a1.double()
        want = v1 + a2.double()
        bar = bar + U * (v1.abs() + bar) + U * (want.abs() + 2 * bar)
    elif option == "colpart":
        item["colpart"] = torch.full(((M + 31) // 32, N), float("nan"), device=DEV)
    (y,) = ops.linear_split_ex([item], M, K, terms=1)
    if option == "add1+add2":
        assert y.data_ptr() == item["out"].data_ptr()
    _check(y, want, bar, option)
    if option == "colpart":                  # 32-row block sums of the stored values: five levels of fp32 additions on top
        pad = (-M) % 32
        blocks = lambda t: F.pad(t, (0, 0, 0, pad)).view(-1, 32, N).sum(1)   # noqa: E731
        _check(item["colpart"], blocks(ref), blocks(bar) + 5 * U * blocks(ref.abs() + bar), "colpart block sums")


# ---- weight gradient ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", WGRAD_SHAPES)
@pytest.mark.parametrize("form", ["plain", "x_pos", "row_keep"])
def test_weight_gradient_vs_float64_of_the_rounded_operands(M, N, K, form):
    """wgrad_bf16r_f32<false, .> and <true, .>: one chunk of few rows and many chunks, one and several tiles; the reduced
    length is M.  Two runs are bit-equal (fixed reduction order)."""
    from egtr_amd import ops
    g, x = operand((M, N), 13, scale=1.0 / 16), operand((M, K), 14)
    kw, xe, ge = {}, x, g
    if form == "x_pos":
        pos_rows = M if M % 2 else M // 2     # 4133 is prime: the table then covers every row
        gen = torch.Generator().manual_seed(15)
        pos = (torch.randint(1, 2 ** 15, (pos_rows, K), generator=gen).double() / 2 ** 18).float()
        xe = x
        x = xe - pos.repeat(M // pos_rows, 1)
        assert torch.equal(x + pos.repeat(M // pos_rows, 1), xe) and not torch.equal(rne(x), rne(xe))
        kw["x_pos"] = pos.to(DEV)
    if form == "row_keep":
        keep = torch.rand(M, generator=torch.Generator().manual_seed(16)) < 0.8
        ge = g * keep.float()[:, None]
        kw["row_keep"] = keep.to(torch.uint8).to(DEV)
    gt, xt = ge.t().contiguous(), xe.t().contiguous()
    if form != "row_keep":
        assert_teeth(gt, xt)                  # (with masked rows the sum is shorter; the plain case carries the teeth)
    ref, bar = product_ref(gt, xt)
    run = lambda: ops._wgrad_ex(g.to(DEV), x.to(DEV), terms=1, **kw)   # noqa: E731
    gw = run()
    _check(gw, ref, bar, f"wgrad {form} {M}x{N}x{K}")
    assert torch.equal(gw, run())
    if form == "plain":
        assert torch.equal(gw, ops.linear_split_bf16_wgrad(g.to(DEV), x.to(DEV), terms=1))


# ---- tiling launches ------------------------------------------------------------------------------------------------------------
def test_tiling_launches_write_the_host_restatements_stream():
    """single, transposed, pair and multi (one entry a row-wise concatenation of two weights) -- bit for bit"""
    from egtr_amd import ops
    w_a, w_b, w_c = operand((256, 256), 61), operand((128, 256), 62), operand((256, 1024), 63)
    w_odd = operand((128, 96), 64)            # K a multiple of 32 only: the single / transposed entries serve it
    host = lambda w: ops.gemm_split_weights(w, terms=1)   # noqa: E731
    same = lambda got, w: got.shape == host(w).shape and torch.equal(_bits(got.cpu()), _bits(host(w)))   # noqa: E731
    assert same(ops.gemm_split_tile(w_odd.to(DEV), terms=1), w_odd)
    assert same(ops.gemm_split_tile(w_c.to(DEV), terms=1), w_c)
    assert same(ops.gemm_split_tile(w_c.to(DEV), transposed=True, terms=1), w_c.t().contiguous())
    wide = torch.zeros(256, 1032, device=DEV)
    wide[:, :1024] = w_c.to(DEV)              # a row-strided weight
    assert same(ops.gemm_split_tile(wide[:, :1024], terms=1), w_c)
    p0, p1 = ops.gemm_split_tile_pair(w_c.to(DEV), terms=1)
    assert same(p0, w_c) and same(p1, w_c.t().contiguous())
    got = ops.gemm_split_tile_pairs([w_a.to(DEV), (w_a.to(DEV), w_b.to(DEV)), w_c.to(DEV)], terms=1)
    for (g0, g1), w in zip(got, (w_a, torch.cat([w_a, w_b], 0), w_c)):
        assert same(g0, w) and same(g1, w.t().contiguous())
    # the two kinds of stream are told apart by their shape
    with pytest.raises(RuntimeError):
        ops.linear_split_bf16(w_a.to(DEV), p0, None, 256, terms=6)
    with pytest.raises(RuntimeError):
        ops.linear_split_bf16(w_a.to(DEV), ops.gemm_split_tile(w_a.to(DEV)), None, 256, terms=1)


# ---- non-finite inputs ------------------------------------------------------------------------------------------------------------
def test_non_finite_elements_stay_in_their_row_or_column():
    from egtr_amd import ops
    M, K, N = 200, 256, 128
    a, w = operand((M, K), 71), operand((N, K), 72, scale=1.0 / 16)
    a[17, 5], a[140, 250] = float("nan"), float("inf")
    y = ops.linear_split_bf16(a.to(DEV), _stream(w, "tile"), None, N, terms=1).cpu()
    bad = ~torch.isfinite(y)
    assert bad[17].all() and bad[140].all() and int(bad.any(1).sum()) == 2
    clean = torch.ones(M, dtype=torch.bool)
    clean[17] = clean[140] = False
    ref, bar = product_ref(a[clean], w)
    _check(y[clean], ref, bar, "the finite rows")
    g = operand((M, N), 73, scale=1.0 / 16)
    gw = ops._wgrad_ex(g.to(DEV), a.to(DEV), terms=1).cpu()      # [N, K]: column k of x -> column k of the gradient
    bad = ~torch.isfinite(gw)
    assert bad[:, 5].all() and bad[:, 250].all() and int(bad.any(0).sum()) == 2
    # a finite value beyond the largest bf16 rounds to inf (documented): its row is non-finite too
    a2 = operand((M, K), 71)
    a2[3, 3] = 3.4e38
    y2 = ops.linear_split_bf16(a2.to(DEV), _stream(w, "tile"), None, N, terms=1).cpu()
    assert (~torch.isfinite(y2)).any(1).nonzero().flatten().tolist() == [3]


# ---- off means off ------------------------------------------------------------------------------------------------------------------
def test_fp32_mode_and_no_block_at_all_are_bit_equal():
    """One forward, one ``ex`` and one wgrad case through TokenLinearFunction / the bindings: inside
    matmul_precision_mode("fp32") and with no block at all the bits are the same, and they are the six-term bits."""
    from egtr_amd import ops
    assert ops.matmul_precision() == "fp32"
    g = torch.Generator().manual_seed(81)
    x = torch.randn(1, 4133, 256, generator=g).to(DEV)
    lin = torch.nn.Linear(256, 256).to(DEV)
    gy = torch.randn(1, 4133, 256, generator=g).to(DEV)

    def run():
        xg = x.clone().requires_grad_(True)
        lin.zero_grad()
        y = ops.TokenLinearFunction.apply(xg, lin.weight, lin.bias, True)
        y.backward(gy)
        return y.detach(), xg.grad, lin.weight.grad.clone(), lin.bias.grad.clone()

    plain = run()
    with ops.matmul_precision_mode("fp32"):
        inside = run()
    for p, q in zip(plain, inside):
        assert torch.equal(p, q)
    wt = ops.gemm_split_tile(lin.weight.detach())
    assert torch.equal(plain[0], ops.linear_split_bf16(x.view(-1, 256), wt, lin.bias, 256, relu=True).view(1, 4133, 256))
    with ops.matmul_precision_mode("bf16"):    # the bindings take ``terms``, not the mode: an inference route keeps its bits
        assert torch.equal(plain[0], ops.linear_split_bf16(x.view(-1, 256), wt, lin.bias, 256, relu=True).view(1, 4133, 256))
        other = run()
    assert not torch.equal(plain[0], other[0]) and not torch.equal(plain[2], other[2])
    x2 = x.view(-1, 256)
    e0 = ops.linear_split_ex([dict(x=x2, wt=wt, N=256, add1=gy.view(-1, 256))], 4133, 256)[0]
    with ops.matmul_precision_mode("fp32"):
        e1 = ops.linear_split_ex([dict(x=x2, wt=wt, N=256, add1=gy.view(-1, 256))], 4133, 256)[0]
        g1 = ops.linear_split_bf16_wgrad(gy.view(-1, 256), x2)
    assert torch.equal(e0, e1) and torch.equal(g1, ops.linear_split_bf16_wgrad(gy.view(-1, 256), x2))


def test_backward_after_the_block_takes_the_route_of_its_forward():
    """forward under "bf16", backward after the block has ended: bit-equal to a backward run inside the block"""
    from egtr_amd import ops
    g = torch.Generator().manual_seed(82)
    x = torch.randn(1, 4133, 256, generator=g).to(DEV)
    lin = torch.nn.Linear(256, 256).to(DEV)
    gy = torch.randn(1, 4133, 256, generator=g).to(DEV)

    def run(backward_inside):
        xg = x.clone().requires_grad_(True)
        lin.zero_grad()
        with ops.matmul_precision_mode("bf16"):
            y = ops.TokenLinearFunction.apply(xg, lin.weight, lin.bias, False)
            if backward_inside:
                y.backward(gy)
        if not backward_inside:
            assert ops.matmul_precision() == "fp32"
            y.backward(gy)
        return xg.grad, lin.weight.grad.clone()

    for p, q in zip(run(True), run(False)):
        assert torch.equal(p, q)
    with ops.matmul_precision_mode("fp32"):
        xg = x.clone().requires_grad_(True)
        ops.TokenLinearFunction.apply(xg, lin.weight, lin.bias, False).backward(gy)
    assert not torch.equal(xg.grad, run(False)[0])


# ---- TokenLinearFunction under the mode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,relu", [(256, False), (1024, True)])
def test_token_linear_function_under_the_mode_vs_float64_autograd(N, relu):
    """x [1, 4133, 256] (4133 >= GEMM_SPLIT_MIN_ROWS).  Output, grad_x, grad_w against float64 autograd of F.linear on the
    RNE-rounded operands (the upstream gradient rounded where it is a GEMM operand), each under its product's derived bar;
    grad_b against the float64 column sum of the UNROUNDED gradient under the fp32 summation bound M 2^-24 sum |g|.  With the
    ReLU, an output within its bar of zero may fall on either side: there the node's own decision is taken."""
    from egtr_amd import ops
    M, K = 4133, 256
    assert M >= ops.GEMM_SPLIT_MIN_ROWS
    g = torch.Generator().manual_seed(91)
    x = torch.randn(1, M, K, generator=g)
    w, b = torch.randn(N, K, generator=g) / 16, torch.randn(N, generator=g)
    gy = torch.randn(1, M, N, generator=g)
    xg = x.to(DEV).requires_grad_(True)
    wp, bp = torch.nn.Parameter(w.to(DEV)), torch.nn.Parameter(b.to(DEV))
    with ops.matmul_precision_mode("bf16"):
        y = ops.TokenLinearFunction.apply(xg, wp, bp, relu)
        y.backward(gy.to(DEV))
    z, zbar = product_ref(x[0], w)
    z = z + b.double()
    zbar = zbar + U * (z.abs() + zbar)
    _check(y[0], z.clamp_min(0) if relu else z, zbar, "output")
    gm = gy[0]
    if relu:
        on = torch.where(z.abs() <= zbar, y[0].detach().cpu() > 0, z > 0)
        gm = gm * on.float()
    x64, w64 = rne(x[0]).double().requires_grad_(True), rne(w).double().requires_grad_(True)
    F.linear(x64, w64).backward(rne(gm).double())
    _check(xg.grad[0], x64.grad, 2.0 * N * U * (rne(gm).double().abs() @ rne(w).double().abs()), "grad_x")
    _check(wp.grad, w64.grad, 2.0 * M * U * (rne(gm).double().abs().t() @ rne(x[0]).double().abs()), "grad_w")
    _check(bp.grad, gm.double().sum(0), M * U * gm.double().abs().sum(0), "grad_b")


# ---- the layer nodes under the mode: measured -----------------------------------------------------------------------------------------
class _RoundedLinear(torch.autograd.Function):
    """fp32 torch statement of a linear whose every product multiplies RNE-bf16-rounded operands: forward r(x) r(w)^T + b,
    data gradient r(g) r(w), weight gradient r(g)^T r(x), bias gradient the column sum of the unrounded g."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return F.linear(rne(x), rne(w), b)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g2, x2 = rne(g).reshape(-1, g.shape[-1]), rne(x).reshape(-1, x.shape[-1])
        return (g2 @ rne(w)).view(x.shape), g2.t() @ x2, g.reshape(-1, g.shape[-1]).sum(0)


def _layer_rounded_fp32(layer, x, pos, ref, mask, shp, lsi):
    """the encoder layer of tests/test_gpu_train_fused.py::_reference_f64 (p = 0) in fp32 with _RoundedLinear for every linear"""
    from egtr_amd.ops import MultiScaleDeformableAttentionFunction
    P = {n: q.detach().clone().requires_grad_(True) for n, q in layer.named_parameters()}
    x, pos = x.clone().requires_grad_(True), pos.clone().requires_grad_(True)
    B, S, _ = x.shape
    lin = _RoundedLinear.apply
    value = lin(x, P["self_attn.value_proj.weight"], P["self_attn.value_proj.bias"])
    value = value.masked_fill(~mask[..., None], 0.0).view(B, S, 8, 32)
    q = x + pos
    off = lin(q, P["self_attn.sampling_offsets.weight"], P["self_attn.sampling_offsets.bias"]).view(B, S, 8, 4, 4, 2)
    aw = F.softmax(lin(q, P["self_attn.attention_weights.weight"], P["self_attn.attention_weights.bias"]).view(B, S, 8, 16),
                   -1).view(B, S, 8, 4, 4)
    norm = torch.stack([shp[..., 1], shp[..., 0]], -1).float()
    loc = ref[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    att = MultiScaleDeformableAttentionFunction.apply(value.contiguous(), shp, lsi, loc.contiguous(), aw.contiguous(), 64)
    a = lin(att.reshape(B, S, 256), P["self_attn.output_proj.weight"], P["self_attn.output_proj.bias"])
    y1 = F.layer_norm(x + a, (256,), P["self_attn_layer_norm.weight"], P["self_attn_layer_norm.bias"], layer.self_attn_layer_norm.eps)
    h = F.relu(lin(y1, P["fc1.weight"], P["fc1.bias"]))
    f = lin(h, P["fc2.weight"], P["fc2.bias"])
    y2 = F.layer_norm(y1 + f, (256,), P["final_layer_norm.weight"], P["final_layer_norm.bias"], layer.final_layer_norm.eps)
    return y2, x, pos, P


ROW_CAP = 0.02    # test_encoder_layer_train_node_vs_float64_reference::close_rows: the share of rows that may be left out


def _rel_err(got, want, rows=False):
    """max-abs error normalised by the float64 tensor's max-abs.  ``rows`` (the gradients that reach the sampling locations,
    judged row by row in tests/test_gpu_train_fused.py because bilinear sampling is not differentiable where a sample crosses a
    pixel boundary): the ROW_CAP share of rows with the largest errors is left out, the same share for every evaluation."""
    want = want.double().reshape(-1, want.shape[-1]) if want.dim() > 1 else want.double().reshape(1, -1)
    err = (got.double().reshape(want.shape) - want).abs().max(1)[0]
    if rows:
        keep = err.numel() - int(ROW_CAP * err.numel())
        err = err.sort()[0][:keep]
    return (err.max() / want.abs().max()).item()


def _assert_measured(errors, no_product=()):
    """errors: name -> (E_fp32 node, E_ref rounded torch composition, E_node one-term node).  E_node <= 2 E_ref: both are
    instances of the same rounding model, and a factor two covers which elements happen to flip; E_ref >= 20 E_fp32: the mode
    does bf16 arithmetic and the comparison can see it.  ``no_product``: tensors that no rounded product reaches (a column sum of the
    upstream gradient: the same launch on the same input in both modes, so neither requirement says anything about the mode;
    the caller asserts that the two nodes agree bit for bit instead)."""
    for name, (e32, eref, enode) in errors.items():
        print(f"{name}: fp32 node {e32:.3e}  rounded torch composition {eref:.3e}  one-term node {enode:.3e}  "
              f"(node / ref {enode / eref:.2f}, ref / fp32 {eref / max(e32, 1e-30):.1f})")
    for name, (e32, eref, enode) in errors.items():
        if name not in no_product:
            assert enode <= 2.0 * eref, (name, enode, eref)
            assert eref >= 20.0 * e32, (name, eref, e32)


def test_encoder_layer_train_node_under_the_mode_measured_against_the_rounding_model():
    """EncoderLayerTrainFunction at B = 1, p = 0 on the 600x1000 pyramid (the smallest case of tests/test_gpu_train_fused.py),
    against that file's float64 layer.  Measured on an MI355X: DESIGN.md 4.12b."""
    from egtr_amd import ops
    from test_gpu_train_fused import _inputs, _layer, _reference_f64
    layer = _layer(dropout=0.0)
    x, pos, ref, mask, shp, lsi, gy = _inputs(1)
    y64, x64, p64, P64 = _reference_f64(layer, x, pos, ref, mask, shp, lsi, None, None, 0.0)
    y64.backward(gy.double())
    want = {"output": y64.detach(), "grad x": x64.grad, "grad pos": p64.grad}
    want.update({f"grad {n}": q.grad for n, q in P64.items()})

    def node(mode):
        layer.zero_grad()
        xg, pg = x.clone().requires_grad_(True), pos.clone().requires_grad_(True)
        with ops.matmul_precision_mode(mode):
            assert ops.encoder_layer_train_supported(layer, xg, pg, ref, mask, False)
            y = ops.encoder_layer_train(layer, xg, mask, pg, ref, shp, lsi, masks=None)
        y.backward(gy)                        # after the block: the node kept its forward's route
        got = {"output": y.detach(), "grad x": xg.grad, "grad pos": pg.grad}
        got.update({f"grad {n}": q.grad.clone() for n, q in layer.named_parameters()})
        return got

    yr, xr, pr, Pr = _layer_rounded_fp32(layer, x, pos, ref, mask, shp, lsi)
    yr.backward(gy)
    got_ref = {"output": yr.detach(), "grad x": xr.grad, "grad pos": pr.grad}
    got_ref.update({f"grad {n}": q.grad for n, q in Pr.items()})
    got32, got16 = node("fp32"), node("bf16")
    rows = ("grad x", "grad pos")
    # the last LayerNorm's bias gradient is the column sum of the upstream gradient: no product, the same launch in both modes
    last = "grad final_layer_norm.bias"
    assert torch.equal(got32[last], got16[last])
    _assert_measured({n: tuple(_rel_err(g[n], want[n], n in rows) for g in (got32, got_ref, got16)) for n in want},
                     no_product=(last,))


def test_decoder_value_projection_node_under_the_mode_measured_against_the_rounding_model():
    """DecoderValueProjTrainFunction at the shapes of tests/test_gpu_train_fused.py (B = 2, S = 4500, six layers, one unused)"""
    from egtr_amd import ops
    g = torch.Generator().manual_seed(21)
    B, S, nl = 2, 4500, 6
    enc = torch.randn(B, S, 256, generator=g).to(DEV)
    mask = (torch.rand(B, S, generator=g) < 0.85).to(DEV)
    lins = [torch.nn.Linear(256, 256).to(DEV) for _ in range(nl)]
    gys = [torch.randn(B, S, 256, generator=g).to(DEV) for _ in range(nl)]
    used = [0, 1, 2, 4, 5]

    class _L:
        def __init__(self, lin):
            self.encoder_attn = type("A", (), {"value_proj": lin})()

    layers = [_L(m) for m in lins]

    def collect(vals, e, params):
        out = {f"values {i}": vals[i].detach() for i in range(nl)}
        out["grad enc"] = e.grad
        for i in used:
            out[f"grad w {i}"], out[f"grad b {i}"] = params[i][0].grad.clone(), params[i][1].grad.clone()
        return out

    def node(mode):
        for m in lins:
            m.zero_grad()
        e = enc.clone().requires_grad_(True)
        with ops.matmul_precision_mode(mode):
            assert ops.decoder_values_train_supported(e, mask, layers)
            vals = ops.decoder_values_train(e, mask, layers)
        sum((vals[i] * gys[i]).sum() for i in used).backward()
        assert lins[3].weight.grad is None
        return collect(vals, e, [(m.weight, m.bias) for m in lins])

    def torch_statement(dtype, linear):
        e = enc.to(dtype).clone().requires_grad_(True)
        P = [(m.weight.detach().to(dtype).requires_grad_(True), m.bias.detach().to(dtype).requires_grad_(True)) for m in lins]
        vals = [linear(e, w, b).masked_fill(~mask[..., None], 0.0) for w, b in P]
        sum((vals[i] * gys[i].to(dtype)).sum() for i in used).backward()
        return collect(vals, e, P)

    want = torch_statement(torch.float64, F.linear)
    got_ref = torch_statement(torch.float32, _RoundedLinear.apply)
    got32, got16 = node("fp32"), node("bf16")
    # a bias gradient is the masked column sum of the upstream gradient: no product, the same launch in both modes
    biases = tuple(f"grad b {i}" for i in used)
    for n in biases:
        assert torch.equal(got32[n], got16[n]), n
    _assert_measured({n: tuple(_rel_err(g[n], want[n]) for g in (got32, got_ref, got16)) for n in want}, no_product=biases)


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
def test_trainer_runs_two_steps_under_the_mode(monkeypatch):
    """DataParallelTrainer(matmul_precision="bf16") on the tiny model of tests/test_gpu_robustness.py with the 320 x 416 images
    of tests/_ddp2_worker.py (2 x 2765 tokens: above the 4096 rows from which the training nodes serve the encoder): losses
    finite, parameters updated, the split-GEMM entries launched with ``terms == 1``, the global setting "fp32" again, ops.FALLBACKS as it was."""
    from egtr_amd import _lib, ops
    from egtr_amd.runtime import DataParallelTrainer, configure_optimizers
    from test_gpu_robustness import _tiny_train_setup
    model, batch = _tiny_train_setup()
    batch = dict(batch, pixel_values=torch.randn(2, 3, 320, 416, generator=torch.Generator().manual_seed(3)).to(DEV),
                 pixel_mask=torch.ones(2, 320, 416, dtype=torch.long, device=DEV))
    assert ops.matmul_precision() == "fp32"
    launched = {}
    real = _lib.launch

    with_terms = {"egtr_linear_split_bf16_ex_f32", "egtr_linear_split_bf16_wgrad_ex_f32", "egtr_gemm_split_tile_weights_f32",
                  "egtr_gemm_split_tile_weights_pair_f32", "egtr_gemm_split_tile_weights_multi_f32"}

    def counting(name, *args, **kw):     # the split-GEMM entries are keyed on (entry, terms): `terms` is their last argument
        key = (name, args[-1]) if name in with_terms else name
        launched[key] = launched.get(key, 0) + 1
        return real(name, *args, **kw)

    fallbacks = dict(ops.FALLBACKS)
    opt = configure_optimizers(model, lr=1e-3, lr_backbone=1e-4, lr_initialized=None)
    tr = DataParallelTrainer(model, optimizer=opt, accumulate=1, clip=0.1, matmul_precision="bf16")
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    monkeypatch.setattr(_lib, "launch", counting)
    for _ in range(2):
        loss, _, stepped = tr.training_step(batch)
        assert stepped and torch.isfinite(loss).item()
        assert ops.matmul_precision() == "fp32"
    tr.finalize()
    moved = [n for n, p in model.named_parameters() if p.requires_grad and not torch.equal(p.detach(), before[n])]
    assert any("encoder" in n and "fc1.weight" in n for n in moved) and len(moved) > 50
    assert all(torch.isfinite(p).all().item() for p in model.parameters())
    assert launched.get(("egtr_linear_split_bf16_ex_f32", 1), 0) > 0
    assert launched.get(("egtr_linear_split_bf16_wgrad_ex_f32", 1), 0) > 0
    assert launched.get(("egtr_gemm_split_tile_weights_multi_f32", 1), 0) > 0
    assert ("egtr_linear_split_bf16_ex_f32", 6) not in launched     # every product of the training nodes took the one-term route
    assert ops.FALLBACKS == fallbacks
