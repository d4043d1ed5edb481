"""CPU: the relation head under the opt-in bf16 matmul precision (egtr_amd.ops.set_matmul_precision) -- the host
restatement of the one-piece weight streams of the one-term training forward (rel_head_fwd_x6<., ., true, 1>,
egtr_amd/csrc/rel_head.hip), the inputs of tests/test_gpu_rel_head_matmul_precision.py with the teeth of their bars, and the
argument validation of the two new C entries.

Arithmetic under the mode: layer 1 is fp32; layer 2 of both MLPs multiplies RNE(W2) by RNE(h1), layer 3 of the relation MLP
RNE(W3) by RNE(h2), each with fp32 accumulation; the connectivity output layer is fp32.  Reference and bar of a rounded product
are those of tests/test_matmul_precision_cpu.py (``product_ref``): the float64 product of the rounded operands, 2 K 2^-24
sum |a_r w_r| per element.

``stage_inputs``.  Gate logits 40 + 40 make every gate exactly 1 (tests/test_gpu_token_x6.py shows it bit for bit); with uk = 0,
b1 = 0 and uq zero except slot 0 the hidden-1 value of pair (i, j) is relu(uq[i, 0, :]) exactly, so layer 2 sees ``operand``
values (a known fraction of a bf16 ulp above a bf16 value) with about 40 % of them cut to zero.  Both W2 are ``operand`` values
with random signs, W3 is all positive; the layer-2 biases are small against sum |a w| (the accumulator starts from the bias, so
a bias of the size of the sum would take a share of the bar that ``product_ref`` does not count)."""
import ctypes

import pytest
import torch

from test_matmul_precision_cpu import assert_teeth, operand, rne

# (B, N, T, R): a partial 8 x 4 pair tile in both directions with OT = 1 and a batch offset (98 rows: three full 32-row colpart
# blocks and a partial one); ragged in both directions with OT = 2 and zero-padded W3 rows; all 64 relation rows live
SHAPES = [(2, 7, 4, 7), (1, 37, 7, 50), (2, 13, 4, 64)]
NAMES = ("gate_q", "gate_k", "uq", "uk", "b1", "w2r", "b2r", "w3r", "b3r", "w2c", "b2c", "w3c", "b3c")


def stage_inputs(B, N, T, R, seed=7):
    """name -> CPU fp32 tensor, in the argument order of the relation-head bindings"""
    g = torch.Generator().manual_seed(seed)
    sign = lambda *s: torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0)   # noqa: E731
    u = operand((B, N, 512), seed + 1)
    uq = torch.zeros(B, N, T, 512)
    uq[:, :, 0] = torch.where(torch.rand(B, N, 512, generator=g) < 0.4, -u, u)
    gate = torch.full((B, N, T), 40.0)
    d = dict(gate_q=gate, gate_k=gate.clone(), uq=uq, uk=torch.zeros(B, N, T, 512), b1=torch.zeros(512),
             w2r=operand((256, 256), seed + 2, scale=1.0 / 16) * sign(256, 256), b2r=torch.randn(256, generator=g) * 0.5,
             w3r=operand((R, 256), seed + 3, scale=1.0 / 16), b3r=torch.randn(R, generator=g) * 0.5,
             w2c=operand((256, 256), seed + 4, scale=1.0 / 16) * sign(256, 256), b2c=torch.randn(256, generator=g) * 0.5,
             w3c=torch.randn(1, 256, generator=g) / 16, b3c=torch.randn(1, generator=g) * 0.5)
    assert tuple(d) == NAMES
    return d


def hidden1(d):
    """[2 (mlp), B N, 256]: the hidden-1 rows of ``stage_inputs`` (one per subject; every object j repeats them)"""
    h = torch.relu(d["uq"][:, :, 0]).reshape(-1, 512)
    return torch.stack([h[:, :256], h[:, 256:]])


def hidden2_one_term(h1, w2, b2):
    """host evaluation of layer 2 of the one-term model: relu(RNE(h1) RNE(W2)^T + b2), summed in float64, as fp32"""
    return torch.relu(rne(h1).double() @ rne(w2).double().t() + b2.double()).float()


# ---- the one-piece streams from their definition --------------------------------------------------------------------------------
def streams_definition(w2, w3):
    """w2x [8 nt][16 t][64 lane][8] = RNE(W2)[32 nt + (lane & 31)][16 t + 8 (lane >> 5) + e];
    w3x [8 nt][2 kb][OT][64 lane][8] = RNE(W3)[32 ot + (lane & 31)][32 nt + 16 kb + (e & 3) + 8 (e >> 2) + 4 (lane >> 5)],
    rows at or beyond num_rel zero -- written element by element from the layout formulas"""
    R = w3.shape[0]
    OT = 1 if R <= 32 else 2
    w2b, w3b = w2.to(torch.bfloat16), w3.to(torch.bfloat16)
    w2x = torch.empty(8, 16, 64, 8, dtype=torch.bfloat16)
    w3x = torch.empty(8, 2, OT, 64, 8, dtype=torch.bfloat16)
    for nt in range(8):
        for lane in range(64):
            for t in range(16):
                for e in range(8):
                    w2x[nt, t, lane, e] = w2b[32 * nt + (lane & 31), 16 * t + 8 * (lane >> 5) + e]
            for kb in range(2):
                for ot in range(OT):
                    for e in range(8):
                        row, col = 32 * ot + (lane & 31), 32 * nt + 16 * kb + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)
                        w3x[nt, kb, ot, lane, e] = w3b[row, col] if row < R else 0.0
    return w2x, w3x


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("R", [7, 50, 64])
def test_one_piece_streams_restatement_against_its_definition(R):
    from egtr_amd import ops
    d = stage_inputs(1, 8, 4, R)
    w2r, w3r, w2c = d["w2r"].clone(), d["w3r"], d["w2c"]
    w2r[3, 7], w2r[130, 40] = float("inf"), float("nan")
    w2r[0, 0], w2r[0, 1] = 3.0e38, 3.4e38         # below / beyond the upper rounding boundary of the largest bf16
    w2r[1, 0] = 1.0 + 2.0 ** -8                    # half way between two bf16 values: to the even one, down
    w2r[1, 1] = 1.0 + 2.0 ** -7 + 2.0 ** -8        # half way between an odd and an even bf16 value: up
    w2xr, w3x, w2xc = ops.rel_head_split_weights(w2r, w3r, w2c, terms=1)
    OT = 1 if R <= 32 else 2
    assert all(t.dtype == torch.bfloat16 and t.is_contiguous() for t in (w2xr, w3x, w2xc))
    assert tuple(w2xr.shape) == tuple(w2xc.shape) == (8, 16, 2, 32, 8) and tuple(w3x.shape) == (8, 2, OT, 2, 32, 8)
    want2, want3 = streams_definition(w2r, w3r)
    assert torch.equal(_bits(w2xr).view(8, 16, 64, 8), _bits(want2))
    assert torch.equal(_bits(w3x).view(8, 2, OT, 64, 8), _bits(want3))
    assert torch.equal(_bits(w2xc).view(8, 16, 64, 8), _bits(streams_definition(w2c, w3r)[0]))
    # W2[3][7]: nt 0, pi 3, t 0, hf 0, e 7;  W2[130][40]: nt 4, pi 2, t 2, hf 1, e 0 -- each stays in its element
    f = w2xr.float()
    assert torch.isinf(f[0, 0, 0, 3, 7]) and torch.isnan(f[4, 2, 1, 2, 0])
    assert int((~torch.isfinite(f)).sum()) == 3    # the Inf, the NaN and the 3.4e38 that rounds to Inf
    assert torch.isfinite(f[0, 0, 0, 0, 0]) and torch.isinf(f[0, 0, 0, 0, 1])
    assert f[0, 0, 0, 1, 0] == 1.0 and f[0, 0, 0, 1, 1] == 1.0 + 2.0 ** -6
    if R < 32 * OT:                                # the padded W3 rows are zero
        assert not w3x.view(8, 2, OT, 2, 32, 8)[:, :, OT - 1, :, R - 32 * (OT - 1):].float().any()
    # the six-term streams are what they were, and the two kinds are told apart by their shape
    s6 = ops.rel_head_split_weights(w2r, w3r, w2c)
    assert tuple(s6[0].shape) == (8, 16, 3, 2, 32, 8) and tuple(s6[1].shape) == (8, 2, OT, 3, 2, 32, 8)
    assert torch.equal(_bits(s6[0]), _bits(ops.rel_head_split_weights(w2r, w3r, w2c, terms=6)[0]))
    with pytest.raises(ValueError):
        ops.rel_head_split_weights(w2r, w3r, w2c, terms=3)


# ---- teeth --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,T,R", SHAPES)
def test_bars_separate_the_one_term_layers_from_their_wrong_neighbours(B, N, T, R):
    """layer 2 of both MLPs (h1, W2) and layer 3 of the relation MLP (h2, W3), h2 from a host evaluation of the one-term model:
    the derived bar tells the RNE product from truncated operands, unrounded operands and a dropped k-step in at least half of
    the elements, with about 40 % of h1 and about half of h2 zero, signed (W2) and positive (W3) weights"""
    d = stage_inputs(B, N, T, R)
    h1 = hidden1(d)
    assert 0.3 < (h1 == 0).double().mean().item() < 0.5
    assert bool((d["w2r"] < 0).any()) and bool((d["w2r"] > 0).any()) and bool((d["w3r"] > 0).all())
    for mlp, (w2, b2) in enumerate((("w2r", "b2r"), ("w2c", "b2c"))):
        assert_teeth(h1[mlp], d[w2])
        h2 = hidden2_one_term(h1[mlp], d[w2], d[b2])
        assert 0.3 < (h2 == 0).double().mean().item() < 0.7
        # the accumulator starts from the bias: it must be small against the sum the bar is made of
        assert bool((d[b2].abs()[None, :] <= 0.25 * (rne(h1[mlp]).abs() @ rne(d[w2]).abs().t())).all())
        if mlp == 0:
            assert_teeth(h2, d["w3r"])


# ---- argument validation --------------------------------------------------------------------------------------------------------------
def test_new_entries_reject_null_operands_without_a_gpu():
    """EGTR_E_ARG for NULL operands, before any HIP call: checkable on a CPU-only machine"""
    from egtr_amd import _lib
    h = _lib.lib()
    E_ARG = -1
    nul = [None] * 15
    assert h.egtr_rel_head_forward_bf16r_save_f32(None, *nul, 1, 8, 4, 256, 7, 0, None, None, None, None, None) == E_ARG
    assert h.egtr_rel_head_streams_bf16r_f32(None, None, None, None, 256, 7, None, None, None) == E_ARG
    # one NULL among otherwise plausible (never dereferenced) host addresses is enough, whichever operand it is
    raw = ctypes.create_string_buffer(64 + 16)
    p = (ctypes.addressof(raw) + 15) & ~15
    for miss in (0, 5, 7, 12):                     # gate_q, w2x_rel, w3x_rel, b3c
        ops_ = [p] * 13 + [None, None]             # triplet_dist / node_cls may be NULL
        ops_[miss] = None
        assert h.egtr_rel_head_forward_bf16r_save_f32(None, *ops_, 1, 8, 4, 256, 7, 0, p, p, None, p, p) == E_ARG
    assert h.egtr_rel_head_forward_bf16r_save_f32(None, *([p] * 13), None, None, 1, 8, 4, 256, 7, 0, p, p, None, p, None) == E_ARG
    assert h.egtr_rel_head_forward_bf16r_save_f32(None, *([p] * 14), None, 1, 8, 4, 256, 7, 12, p, p, None, p, p) == E_ARG
    for miss in range(6):
        a = [p] * 6
        a[miss] = None
        assert h.egtr_rel_head_streams_bf16r_f32(None, a[0], a[1], a[2], 256, 7, a[3], a[4], a[5]) == E_ARG
    assert h.egtr_rel_head_streams_bf16r_f32(None, p, p, p, 256, 0, p, p, p) == E_ARG
    # shapes the kernels do not serve: EGTR_E_UNSUPPORTED, again before any HIP call
    E_UNSUPPORTED = -3
    for slots, hidden, rel in ((5, 256, 7), (4, 128, 7), (4, 256, 65)):
        assert h.egtr_rel_head_forward_bf16r_save_f32(None, *([p] * 13), None, None, 1, 8, slots, hidden, rel, 0, p, p, None,
                                                      p, p) == E_UNSUPPORTED
    assert h.egtr_rel_head_streams_bf16r_f32(None, p, p, p, 128, 7, p, p, p) == E_UNSUPPORTED
    assert h.egtr_rel_head_streams_bf16r_f32(None, p, p, p, 256, 65, p, p, p) == E_UNSUPPORTED
    assert h.egtr_abi_version() == 7               # the ABI number these signatures belong to
