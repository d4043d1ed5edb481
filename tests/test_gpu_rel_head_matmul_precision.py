"""GPU (-m gpu): the relation head's training kernels under the opt-in bf16 matmul precision (egtr_amd.ops.set_matmul_precision,
DESIGN.md 4.12b): the one-term forward rel_head_fwd_x6<., ., true, 1> on one-piece weight streams (egtr_amd/csrc/rel_head.hip)
through ``ops.relation_head_train_forward(terms=1)``, and ``ops.RelationHeadFunction`` under the mode, whose backward takes its
two layer-2 products per MLP through the one-term split-GEMM entries.

The forward is checked STAGE BY STAGE against float64 with the derived bar of tests/test_matmul_precision_cpu.py (2 K 2^-24
sum |a_r w_r| against the float64 product of the RNE-rounded operands, + one fp32 rounding per epilogue addend), each stage fed
with the kernel's own saved activations so that a last-bit difference upstream cannot flip a rounding downstream.  The Function
chains products through ReLU masks: it is MEASURED against the rounding model, as the layer nodes of
tests/test_gpu_matmul_precision.py are."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_matmul_precision import _assert_measured, _bits, _check, _rel_err, _RoundedLinear
from test_matmul_precision_cpu import U, assert_teeth, product_ref, rne
from test_rel_head_matmul_precision_cpu import NAMES, SHAPES, stage_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 11   # object classes of the frequency bias


def _dev(d):
    return [d[n].to(DEV) for n in NAMES]


def _freq_bias(B, N, R, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(C + 1, C + 1, R, generator=g), torch.randint(0, C + 1, (B, N), generator=g)


def _gather_bias(trip, node):
    return torch.stack([trip[node[b]][:, node[b]] for b in range(node.shape[0])], 0)     # [B, N, N, R]


# ---- 1. the forward kernel, stage by stage ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,T,R", SHAPES)
def test_one_term_forward_stage_by_stage_vs_float64_of_the_rounded_operands(B, N, T, R):
    """Every gate is exactly 1, uk = 0, b1 = 0, uq lives in slot 0 only: h1_save[i, j] = relu(uq[i, 0]) BIT FOR BIT.  Then, each
    from the kernel's own saved input: h2_save = relu(RNE(h1_save) RNE(W2)^T + b2) for both MLPs, rel = RNE(h2_save[0]) RNE(W3)^T
    + b3 + frequency bias, conn = h2_save[1] . w3c + b3c in fp32 (unrounded).  The same call with terms=6 -- the switch ignored,
    on the device -- is outside the layer-2 bar in at least half of the elements that the ReLU passes (where it cuts both
    results to zero there is nothing to compare: about half of h2)."""
    from egtr_amd import ops
    d = stage_inputs(B, N, T, R)
    trip, node = _freq_bias(B, N, R, 5)
    P_ = B * N * N
    rel, conn, gm, h1s, h2s = ops.relation_head_train_forward(*_dev(d), trip.to(DEV), node.to(DEV), True, 1)
    assert tuple(rel.shape) == (B, N, N, R) and tuple(conn.shape) == (B, N, N) and tuple(gm.shape) == (T,)
    assert tuple(h1s.shape) == tuple(h2s.shape) == (2, P_, 256) and h1s.dtype == h2s.dtype == torch.float32
    blocks = B * ((N + 7) // 8) * ((N + 3) // 4)
    assert float((gm - 1).abs().max()) <= 2 * blocks * U, gm       # every gate is 1: the mean is a sum of rounded quotients
    want_h1 = torch.relu(d["uq"][:, :, 0]).view(B, N, 1, 2, 256).expand(B, N, N, 2, 256).permute(3, 0, 1, 2, 4).reshape(2, P_, 256)
    assert torch.equal(h1s.cpu().view(torch.int32), want_h1.contiguous().view(torch.int32))
    h1, h2 = h1s.cpu(), h2s.cpu()
    live_share = []
    for mlp, (w2, b2) in enumerate((("w2r", "b2r"), ("w2c", "b2c"))):
        assert_teeth(h1[mlp], d[w2])
        ref, bar = product_ref(h1[mlp], d[w2])
        v = ref + d[b2].double()
        bar2 = bar + U * (v.abs() + bar)
        _check(h2[mlp], v.clamp_min(0), bar2, f"layer 2, mlp {mlp}")
        live_share.append((v, bar2))
    assert_teeth(h2[0], d["w3r"])
    ref, bar = product_ref(h2[0], d["w3r"])
    v1 = ref + d["b3r"].double()
    v2 = v1 + _gather_bias(trip, node).double().reshape(P_, R)
    _check(rel.reshape(P_, R), v2, bar + U * (ref.abs() + bar) + U * (v1.abs() + bar) + U * (v2.abs() + bar), "layer 3, relation")
    terms = h2[1].double() * d["w3c"].double()
    vc = terms.sum(1) + d["b3c"].double()
    _check(conn.reshape(P_), vc, 256 * U * (terms.abs().sum(1) + d["b3c"].double().abs()), "layer 3, connectivity (fp32)")
    # the neighbour on the device: six terms are fp32-accurate, i.e. the product of the UNROUNDED operands
    h2_six = ops.relation_head_train_forward(*_dev(d), trip.to(DEV), node.to(DEV), True, 6)[4].cpu()
    for mlp, (v, bar2) in enumerate(live_share):
        live = v > bar2
        assert 0.3 < live.double().mean().item() < 0.7
        share = ((h2_six[mlp].double() - v.clamp_min(0)).abs() > bar2)[live].double().mean().item()
        print(f"terms=6 outside the layer-2 bar, mlp {mlp}: {share:.3f} of the live elements")
        assert share >= 0.5, (mlp, share)


# ---- 2. the streams -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [7, 50, 64])
def test_one_piece_streams_launch_writes_the_host_restatement(R):
    from egtr_amd import ops
    B, N, T = 2, 7, 4
    d = stage_inputs(B, N, T, R)
    d["w2r"][3, 7], d["w2r"][130, 40], d["w3r"][R - 1, 255] = float("inf"), float("nan"), 3.4e38
    host = ops.rel_head_split_weights(d["w2r"], d["w3r"], d["w2c"], terms=1)
    dev = ops.rel_head_streams(d["w2r"].to(DEV), d["w3r"].to(DEV), d["w2c"].to(DEV), terms=1)
    for a, b in zip(host, dev):        # bit for bit; a NaN is a NaN in the same element (its payload is the cast's own choice)
        b = b.cpu()
        nan = torch.isnan(a)
        assert a.shape == b.shape and b.dtype == torch.bfloat16 and torch.equal(nan, torch.isnan(b))
        assert torch.equal(_bits(a).masked_fill(nan, 0), _bits(b).masked_fill(nan, 0))
    assert int(torch.isnan(host[0]).sum()) == 1 and int(torch.isinf(host[0]).sum()) == 1 and int(torch.isinf(host[1]).sum()) == 1
    d = stage_inputs(B, N, T, R)                 # finite weights again: the forward with either stream gives equal bits
    host = [t.to(DEV) for t in ops.rel_head_split_weights(d["w2r"], d["w3r"], d["w2c"], terms=1)]
    a = ops.relation_head_train_forward(*_dev(d), None, None, False, 1, streams=host)
    b = ops.relation_head_train_forward(*_dev(d), None, None, False, 1)
    assert a[2] is None and b[2] is None
    for x, y in zip((a[0], a[1], a[3], a[4]), (b[0], b[1], b[3], b[4])):
        assert torch.equal(x, y)
    with pytest.raises(RuntimeError):            # the two kinds of stream are told apart by their shape
        ops.relation_head_train_forward(*_dev(d), None, None, False, 6, streams=host)


# ---- 3. the Function under the mode: measured ---------------------------------------------------------------------------------------
class _RoundedForwardLinear(torch.autograd.Function):
    """forward r(x) r(w)^T + b; backward of the UNROUNDED linear (the relation output layer: its gradients stay fp32)"""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return F.linear(rne(x), rne(w), b)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g2, x2 = g.reshape(-1, g.shape[-1]), x.reshape(-1, x.shape[-1])
        return (g2 @ w).view(x.shape), g2.t() @ x2, g2.sum(0)


def _head_rounded_fp32(gate_q, gate_k, uq, uk, b1, w2r, b2r, w3r, b3r, w2c, b2c, w3c, b3c, bias):
    """tests/cpu_kernels.relation_head in fp32 with exactly the products of the mode rounded: layer 2 of both MLPs (forward,
    data gradient, weight gradient), layer 3 of the relation MLP in the forward only"""
    g = torch.sigmoid(gate_q[:, :, None, :] + gate_k[:, None, :, :])
    h1 = torch.relu(torch.einsum("bijt,bitc->bijc", g, uq) + torch.einsum("bijt,bjtc->bijc", g, uk) + b1)
    rel = _RoundedForwardLinear.apply(torch.relu(_RoundedLinear.apply(h1[..., :256], w2r, b2r)), w3r, b3r) + bias
    conn = F.linear(torch.relu(_RoundedLinear.apply(h1[..., 256:], w2c, b2c)), w3c, b3c)
    return rel, conn


def _generic(B, N, T, R, seed):
    from test_gpu_kernels import _head_inputs
    d, trip, node = _head_inputs(seed, B, N, T, R, C)
    g = torch.Generator().manual_seed(seed)
    return d, trip, node, torch.randn(B, N, N, R, generator=g), torch.randn(B, N, N, 1, generator=g)


def _run_function(d, trip, node, g_rel, g_conn, mode, want_gm=True, backward_inside=True, deterministic=False):
    """name -> tensor: the outputs and the 13 gradients of ops.RelationHeadFunction under ``mode``"""
    from egtr_amd import ops
    leaves = [d[n].to(DEV).requires_grad_(True) for n in NAMES]
    td = (trip.to(DEV), node.to(DEV)) if trip is not None else (None, None)
    with ops.deterministic(deterministic):
        if mode is None:
            rel, conn, gm = ops.RelationHeadFunction.apply(*leaves, *td, want_gm)
            torch.autograd.backward([rel, conn], [g_rel.to(DEV), g_conn.to(DEV)])
        else:
            with ops.matmul_precision_mode(mode):
                rel, conn, gm = ops.RelationHeadFunction.apply(*leaves, *td, want_gm)
                if backward_inside:
                    torch.autograd.backward([rel, conn], [g_rel.to(DEV), g_conn.to(DEV)])
            if not backward_inside:
                torch.autograd.backward([rel, conn], [g_rel.to(DEV), g_conn.to(DEV)])
    out = {"rel": rel.detach(), "conn": conn.detach()}
    if want_gm:
        out["gate_mean"] = gm.detach()
    out.update({f"grad {n}": t.grad for n, t in zip(NAMES, leaves)})
    return out


@pytest.mark.parametrize("B,N,T,R", SHAPES)
def test_function_under_the_mode_measured_against_the_rounding_model(B, N, T, R):
    """Outputs and all 13 gradients of RelationHeadFunction under "fp32", under "bf16", and of the rounded fp32 torch composition,
    each against float64 autograd of tests/cpu_kernels.relation_head: E_node <= 2 E_ref, and E_ref >= 20 E_fp32 wherever a
    rounded product lies on the tensor's backward path (w3r, w3c, b2r, b2c see the mode only through the forward's h2: the
    first condition alone).  b3r, b3c: column sums of the upstream gradient, bit-equal between the modes.  gate_mean: the same
    instructions in both kernels, summed by fp32 atomics whose order the hardware chooses -- equal to within that reordering
    (one rounding per workgroup), not bit for bit."""
    import cpu_kernels as ck
    d, trip, node, g_rel, g_conn = _generic(B, N, T, R, 300 + N)
    leaves64 = [d[n].double().requires_grad_(True) for n in NAMES]
    rel64, conn64, gm64 = ck.relation_head(*leaves64, trip.double(), node, True)
    torch.autograd.backward([rel64, conn64], [g_rel.double(), g_conn.double()])
    want = {"rel": rel64.detach(), "conn": conn64.detach()}
    want.update({f"grad {n}": t.grad for n, t in zip(NAMES, leaves64)})
    leaves = [d[n].clone().requires_grad_(True) for n in NAMES]
    relr, connr = _head_rounded_fp32(*leaves, _gather_bias(trip, node))
    torch.autograd.backward([relr, connr], [g_rel, g_conn])
    got_ref = {"rel": relr.detach(), "conn": connr.detach()}
    got_ref.update({f"grad {n}": t.grad for n, t in zip(NAMES, leaves)})
    got32 = {k: v.cpu() for k, v in _run_function(d, trip, node, g_rel, g_conn, "fp32").items()}
    got16 = {k: v.cpu() for k, v in _run_function(d, trip, node, g_rel, g_conn, "bf16").items()}
    for n in ("grad b3r", "grad b3c"):
        assert torch.equal(got32[n], got16[n]), n
    blocks = B * ((N + 7) // 8) * ((N + 3) // 4)
    assert float((got32["gate_mean"] - got16["gate_mean"]).abs().max()) <= 2 * blocks * U
    assert float((got16["gate_mean"].double() - gm64.detach()).abs().max()) <= 1e-5
    forward_only = ("grad w3r", "grad w3c", "grad b2r", "grad b2c")
    errors = {n: tuple(_rel_err(g[n], want[n]) for g in (got32, got_ref, got16)) for n in want
              if n not in ("grad b3r", "grad b3c")}
    _assert_measured({n: e for n, e in errors.items() if n not in forward_only})
    for n in forward_only:
        e32, eref, enode = errors[n]
        print(f"{n}: fp32 node {e32:.3e}  rounded torch composition {eref:.3e}  one-term node {enode:.3e}  "
              f"(node / ref {enode / eref:.2f}, ref / fp32 {eref / max(e32, 1e-30):.1f})")
        assert enode <= 2.0 * eref, (n, enode, eref)


# ---- 4. route and launch evidence -------------------------------------------------------------------------------------------------------
_WITH_TERMS = {"egtr_linear_split_bf16_ex_f32", "egtr_linear_split_bf16_wgrad_ex_f32", "egtr_gemm_split_tile_weights_f32"}
_NEW = ("egtr_rel_head_forward_bf16r_save_f32", "egtr_rel_head_streams_bf16r_f32")


def _counted(monkeypatch, run):
    """(what ``run`` returns, the list of launches: entry names, the split-GEMM entries as (entry, terms))"""
    from egtr_amd import _lib
    real, seen = _lib.launch, []

    def counting(name, *args, **kw):
        seen.append((name, args[-1]) if name in _WITH_TERMS else name)
        return real(name, *args, **kw)

    with monkeypatch.context() as m:
        m.setattr(_lib, "launch", counting)
        out = run()
    return out, seen


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for n in a:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("B,N,T,R", SHAPES)
def test_route_and_launches_under_each_mode(monkeypatch, B, N, T, R):
    from egtr_amd import ops
    assert ops.matmul_precision() == "fp32" and ops.REL_HEAD_TRAIN_X6 and ops.GEMM_SPLIT_BF16 and ops.GEMM_SPLIT_WGRAD
    d, trip, node, g_rel, g_conn = _generic(B, N, T, R, 400 + N)
    fallbacks = dict(ops.FALLBACKS)
    # gate_mean is summed by atomics (order-dependent bits): left out where bits are compared
    run = lambda mode: _counted(monkeypatch, lambda: _run_function(d, trip, node, g_rel, g_conn, mode, want_gm=False))   # noqa: E731
    got16, seen16 = run("bf16")
    assert seen16.count("egtr_rel_head_forward_bf16r_save_f32") == 1 and seen16.count("egtr_rel_head_streams_bf16r_f32") == 1
    assert seen16.count(("egtr_linear_split_bf16_ex_f32", 1)) == 2
    assert seen16.count(("egtr_linear_split_bf16_wgrad_ex_f32", 1)) == 2
    assert seen16.count(("egtr_gemm_split_tile_weights_f32", 1)) == 2
    assert "egtr_rel_head_forward_bf16x6_save_f32" not in seen16 and "egtr_rel_head_streams_f32" not in seen16
    assert not [s for s in seen16 if isinstance(s, tuple) and s[1] != 1]
    got32, seen32 = run("fp32")
    got_plain, seen_plain = run(None)
    assert seen32 == seen_plain and not [s for s in seen32 if s in _NEW]
    assert seen32.count("egtr_rel_head_forward_bf16x6_save_f32") == 1
    assert seen32.count(("egtr_linear_split_bf16_wgrad_ex_f32", 6)) == 2 and ("egtr_linear_split_bf16_ex_f32", 6) not in seen32
    _same_bits(got32, got_plain)
    assert not torch.equal(got32["rel"], got16["rel"]) and not torch.equal(got32["grad uq"], got16["grad uq"])
    assert ops.FALLBACKS == fallbacks


def test_unserved_slot_count_takes_the_exact_f32_route_under_either_mode(monkeypatch):
    """T = 5: neither split kernel serves it; under "bf16" the exact-f32 entry runs and forward and backward keep their fp32 bits"""
    from egtr_amd import ops
    d, trip, node, g_rel, g_conn = _generic(2, 13, 5, 50, 450)
    fallbacks = dict(ops.FALLBACKS)
    got16, seen16 = _counted(monkeypatch, lambda: _run_function(d, trip, node, g_rel, g_conn, "bf16", want_gm=False))
    got32, seen32 = _counted(monkeypatch, lambda: _run_function(d, trip, node, g_rel, g_conn, "fp32", want_gm=False))
    assert seen16 == seen32 and seen16.count("egtr_rel_head_forward_save_f32") == 1
    assert not [s for s in seen16 if s in _NEW or (isinstance(s, tuple) and s[1] == 1)]
    _same_bits(got16, got32)
    assert ops.FALLBACKS == fallbacks


# ---- 5. backward after the block ----------------------------------------------------------------------------------------------------
def test_backward_after_the_block_takes_the_route_of_its_forward():
    from egtr_amd import ops
    d, trip, node, g_rel, g_conn = _generic(2, 13, 4, 64, 500)
    inside = _run_function(d, trip, node, g_rel, g_conn, "bf16", want_gm=False)
    after = _run_function(d, trip, node, g_rel, g_conn, "bf16", want_gm=False, backward_inside=False)
    assert ops.matmul_precision() == "fp32"
    _same_bits(inside, after)
    fp32 = _run_function(d, trip, node, g_rel, g_conn, "fp32", want_gm=False)
    for n in ("grad uq", "grad uk", "grad gate_q", "grad w2r", "grad w2c", "grad b1"):
        assert not torch.equal(fp32[n], after[n]), n


# ---- 6. determinism -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,T,R", SHAPES)
def test_two_runs_under_the_mode_and_deterministic_mode_are_bit_equal(B, N, T, R):
    """no gate_mean buffer (the model reduces the gate means itself under the mode); the ``ex`` and weight-gradient entries sum in
    a fixed order"""
    d, trip, node, g_rel, g_conn = _generic(B, N, T, R, 600 + N)
    a = _run_function(d, trip, node, g_rel, g_conn, "bf16", want_gm=False, deterministic=True)
    b = _run_function(d, trip, node, g_rel, g_conn, "bf16", want_gm=False, deterministic=True)
    _same_bits(a, b)


# ---- 7. non-finite values stay where they belong ------------------------------------------------------------------------------------
def test_non_finite_values_stay_in_their_rows_and_columns():
    """An Inf in one uq row (relation half): the relation logits of that subject's pairs are non-finite, no other output is.
    A NaN in one element (p, r) of grad_rel: row p of the ``ex`` input, so row p of dh1 (the gradients of subject i's / object
    j's tables and gate logits and nobody else's) and the weight-gradient rows / column sums of the RELATION MLP's live hidden-2
    units, since each sums over row p; W3's gradient and b3's only in row / element r (fp32 products of column r); the
    connectivity MLP, which shares no product with it, stays finite throughout."""
    B, N, T, R = 2, 13, 4, 7
    d, trip, node, g_rel, g_conn = _generic(B, N, T, R, 700)
    d_inf = {k: v.clone() for k, v in d.items()}
    d_inf["uq"][1, 5, 2, 100] = float("inf")
    out = {k: v.cpu() for k, v in _run_function(d_inf, trip, node, g_rel, g_conn, "bf16", want_gm=False).items()}
    bad = ~torch.isfinite(out["rel"])
    assert bad[1, 5].all() and int(bad.sum()) == N * R
    assert torch.isfinite(out["conn"]).all()
    g_nan = g_rel.clone()
    b, i, j, r = 1, 4, 9, 3
    g_nan[b, i, j, r] = float("nan")
    out = {k: v.cpu() for k, v in _run_function(d, trip, node, g_nan, g_conn, "bf16", want_gm=False).items()}
    assert torch.isfinite(out["rel"]).all() and torch.isfinite(out["conn"]).all()
    bad = {n: ~torch.isfinite(out[f"grad {n}"]) for n in NAMES}
    assert bad["w3r"][r].all() and int(bad["w3r"].any(1).sum()) == 1
    assert bad["b3r"].nonzero().flatten().tolist() == [r]
    # dh2[p, n] is NaN where the ReLU of hidden-2 unit n passed pair p (a select, not a product): the rows n of W2's gradient
    units = bad["b2r"]
    assert units.any() and torch.equal(bad["w2r"], units[:, None].expand(256, 256)) and bad["b1"][:256].any()
    for n in ("w2c", "b2c", "w3c", "b3c"):
        assert not bad[n].any(), n
    assert not bad["b1"][256:].any()
    for n, row in (("uq", i), ("uk", j), ("gate_q", i), ("gate_k", j)):
        rows = bad[n].reshape(B, N, -1).any(-1)
        assert rows[b, row] and int(rows.sum()) == 1, n
    assert not bad["uq"][..., 256:].any() and not bad["uk"][..., 256:].any()
