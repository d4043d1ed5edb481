"""GPU (-m gpu): the deterministic mode (``egtr_amd.ops.deterministic``).

* MSDA backward: five runs of every kernel path give one bit pattern; every result meets the criteria of the default route
  against the oracle; the scale logic (2^+-40, all-zero, inf, float64); the default route is untouched.
* Relation loss: ties at the selection threshold are taken lowest flat index first (numpy restatement in
  tests/test_deterministic_cpu.py), dense and bit-packed entries.
* Gate means, and a model segment (encoder + decoder + heads + loss, forward and backward) run twice from the same seed.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import helpers as Hh
import weights as W
from oracle import loss as OL
from oracle import msda as OM
from test_deterministic_cpu import relation_selection  # noqa: F401  (the restatement's long-standing import path)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PYRAMID = [(19, 32), (10, 16), (5, 8), (3, 4)]
DEC_PYRAMID = [(38, 63), (19, 32), (10, 16), (5, 8)]


def _kernels():
    from egtr_amd.load_custom import load_hip_kernels
    return load_hip_kernels()


def _grid_inputs(*a):
    import test_gpu_kernels as GK
    return GK._grid_inputs(*a)


def _contention():
    """Every sampling location of every query at ONE off-centre point: on level 0 all Lq * P contributions of a head land on
    the same four pixels (and on four pixels of each other level)."""
    x = dict(_grid_inputs(9, 2, PYRAMID, 1.0))
    loc = torch.empty_like(x["loc"])
    loc[..., 0], loc[..., 1] = 0.4031, 0.6127
    x["loc"] = loc
    return x


def _bf16(x):
    x = dict(x)
    x["value"], x["grad_out"] = x["value"].to(torch.bfloat16), x["grad_out"].to(torch.bfloat16)
    return x


CASES = {
    # name: (inputs, what it exercises)
    "encoder": lambda: _grid_inputs(9, 2, PYRAMID, 1.0),                                   # S = Lq = 820: tile pair
    "below256": lambda: _grid_inputs(9, 3, [(9, 13), (5, 7)], 0.5),                        # Lq = S = 152 < 256: per-sample route
    "decoder": lambda: W.make_msda_inputs(14, 2, 300, 8, 32, DEC_PYRAMID, 4, oob_frac=0.2),   # four waves per query
    "decoder_long": lambda: W.make_msda_inputs(14, 1, 5000, 8, 32, DEC_PYRAMID, 4, oob_frac=0.2),   # nq * 4 > 16384
    "generic": lambda: W.make_msda_inputs(7, 2, 13, 3, 20, [(6, 5), (2, 3)], 2),           # variant 3
    "contention": _contention,
    "encoder_bf16": lambda: _bf16(_grid_inputs(9, 2, PYRAMID, 1.0)),
    "decoder_bf16": lambda: _bf16(W.make_msda_inputs(14, 2, 300, 8, 32, DEC_PYRAMID, 4, oob_frac=0.2)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(host inputs, oracle gradients): built once, left unchanged."""
    x = CASES[name]()
    ref = OM.msda_backward(x["value"].float(), x["shapes"], x["lsi"], x["loc"], x["attn"], x["grad_out"].float())
    return x, ref


def backward(x, deterministic, **override):
    from egtr_amd import ops
    d = {n: t.to(DEV) for n, t in dict(x, **override).items()}
    with ops.deterministic(deterministic):
        out = _kernels().ms_deform_attn_backward(d["value"], d["shapes"], d["lsi"], d["loc"], d["attn"], d["grad_out"], 64)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def check_against_oracle(name, got, ref):
    gv, gl, ga = got
    rgv, rgl, rga = ref
    errs = dict(grad_value=float((gv.float() - rgv).abs().max()), grad_attn=float((ga - rga).abs().max()),
                grad_loc=float((gl - rgl).abs().max()))
    print(name, errs)
    if name.endswith("bf16"):   # the criteria of test_msda_bf16_backward
        assert errs["grad_value"] < 2 ** -7 * max(1.0, float(rgv.abs().max()))
        assert errs["grad_attn"] < 1e-3 * max(1.0, float(rga.abs().max()))
        assert errs["grad_loc"] < 1e-3 * max(1.0, float(rgl.abs().max()))
    else:                       # the criteria of test_msda_backward_tile_variant
        assert errs["grad_value"] < 3e-4 * max(1.0, float(rgv.abs().max()))
        assert errs["grad_attn"] < 2e-4
        assert errs["grad_loc"] < 5e-3 * max(1.0, float(rgl.abs().max()) / 50)


@pytest.mark.parametrize("name", list(CASES))
def test_msda_backward_is_reproducible_and_meets_the_oracle(name):
    x, ref = case(name)
    runs = [backward(x, True) for _ in range(5)]
    for r in runs[1:]:
        for a, b, what in zip(runs[0], r, ("grad_value", "grad_loc", "grad_attn")):
            assert torch.equal(a, b), what
    assert runs[0][0].dtype == x["value"].dtype and float(runs[0][0].float().abs().max()) > 0
    check_against_oracle(name, runs[0], ref)


@pytest.mark.parametrize("name", ["encoder", "below256", "decoder", "decoder_long", "generic", "contention", "decoder_bf16"])
def test_mode_off_is_untouched(name):
    """grad_loc / grad_attn never depended on an order: the default call returns the deterministic call's bits; its grad_value
    meets the same criteria."""
    x, ref = case(name)
    det, off = backward(x, True), backward(x, False)
    assert torch.equal(det[1], off[1]) and torch.equal(det[2], off[2])
    check_against_oracle(name, off, ref)


@pytest.mark.parametrize("name", ["encoder", "contention"])
def test_msda_scale_logic(name):
    x, _ = case(name)
    base = backward(x, True)[0]
    for j in (40, -40):
        gv = backward(x, True, grad_out=x["grad_out"] * 2.0 ** j)[0]
        assert torch.isfinite(gv).all()
        assert torch.equal(gv * 2.0 ** -j, base), j          # exact: a power of two, far from the ends of the fp32 range
    zero = backward(x, True, grad_out=torch.zeros_like(x["grad_out"]))[0]
    assert torch.equal(zero, torch.zeros_like(zero))
    go = x["grad_out"].clone()
    go[1, 17, 5] = float("inf")
    gv, gl, ga = backward(x, True, grad_out=go)
    assert torch.isnan(gv).all()
    at = x["attn"].clone()
    at[0, 3, 2, 1, 0] = float("nan")
    assert torch.isnan(backward(x, True, attn=at)[0]).all()


def test_float64_raises_under_the_mode_only():
    x = W.make_msda_inputs(7, 1, 5, 3, 20, [(6, 5), (2, 3)], 2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="ms_deform_attn_backward does not have a deterministic implementation"):
        backward(x, True)
    gv, gl, ga = backward(x, False)
    assert gv.dtype == torch.float64 and torch.isfinite(gv).all()


def test_c_entry_clears_its_outputs_and_workspace_itself():
    """egtr_msda_backward_det_f32 on NaN-filled outputs and a NaN-filled workspace, encoder-shaped (accumulator rows cleared in
    the first kernel) and decoder-shaped (memset): the bits of the call through the module."""
    from egtr_amd import _lib, ops
    lib = _lib.lib()
    for name in ("encoder", "decoder"):
        x, _ = case(name)
        want = backward(x, True)
        d = {n: t.to(DEV) for n, t in x.items()}
        B, S, M, D = d["value"].shape
        Lq, L, P = d["loc"].shape[1], d["shapes"].shape[0], d["loc"].shape[4]
        nbytes = int(lib.egtr_msda_backward_det_workspace_bytes(B, S, M, D))
        assert nbytes == 64 + 8 * B * S * M * D
        ws = torch.full((nbytes // 4,), float("nan"), device=DEV)
        gv, gl, ga = (torch.full_like(d[k], float("nan")) for k in ("value", "loc", "attn"))
        _lib.check(lib.egtr_msda_backward_det_f32(ops._stream(), d["grad_out"].data_ptr(), d["value"].data_ptr(),
                                                  d["shapes"].data_ptr(), d["lsi"].data_ptr(), d["loc"].data_ptr(),
                                                  d["attn"].data_ptr(), B, S, M, D, L, Lq, P, gv.data_ptr(), gl.data_ptr(),
                                                  ga.data_ptr(), ws.data_ptr()), "msda backward det")
        torch.cuda.synchronize()
        for a, b in zip(want, (gv, gl, ga)):
            assert torch.equal(a, b.cpu())
        assert lib.egtr_msda_backward_det_f32(ops._stream(), d["grad_out"].data_ptr(), d["value"].data_ptr(),
                                              d["shapes"].data_ptr(), d["lsi"].data_ptr(), d["loc"].data_ptr(),
                                              d["attn"].data_ptr(), B, S, M, D, L, Lq, P, gv.data_ptr(), gl.data_ptr(),
                                              ga.data_ptr(), None) == -1


# ------------------------------------------------------------------------------------------------------------- loss ties
K_TIE = 2


@functools.lru_cache(maxsize=None)
def tie_case():
    """B = 2, N = 24, R = 5, logits from {-0.5, 0, 0.5}: far more candidates share the threshold logit than are needed."""
    import test_gpu_rel_targets as RT
    B, N, R = 2, 24, 5
    g = torch.Generator().manual_seed(2024)
    pred_rel = (torch.randint(0, 3, (B, N, N, R), generator=g).float() - 1.0) * 0.5
    pred_conn = torch.randn(B, N, N, 1, generator=g)
    trips, indices, costs = [], [], []
    for T, K in ((6, 4), (5, 3)):
        so = torch.stack([torch.randint(0, T, (K,), generator=g), torch.randint(0, T, (K,), generator=g)], 1)
        trips.append(torch.cat([so, torch.randint(0, R, (K, 1), generator=g)], 1))
        indices.append((torch.randperm(N, generator=g)[:T].sort()[0], torch.randperm(T, generator=g)))
        costs.append(torch.randn(T, generator=g) * 3)
    dense = [RT.dense_reference_way(t, N, R) for t in trips]
    return dict(B=B, N=N, R=R, pred_rel=pred_rel, pred_conn=pred_conn, trips=trips, indices=indices, costs=costs, dense=dense)


def tie_expectation(c):
    """float64 numpy: (grad_rel [B, N, N, R], loss_rel, per-image tie info, mult) under the lowest-index-first rule."""
    from loss_restated import relation_expectation
    e = relation_expectation(c, K_TIE, K_TIE, order="key")
    return e.grad, e.loss_rel, e.info, e.mult


def test_loss_ties_are_taken_lowest_index_first():
    import test_gpu_rel_targets as RT
    from egtr_amd import ops, targets as T
    c = tie_case()
    want_grad, want_loss, infos, mult = tie_expectation(c)
    for info in infos:                       # both problems of both images: more tied candidates than needed
        for k, tied, need in info:
            assert k > 0 and 0 < need < tied, infos
    pr, pc = c["pred_rel"].to(DEV), c["pred_conn"].to(DEV)
    pi, ti, mc, off = RT.matcher_flat(c["indices"], c["costs"])
    nm = float(OL.nonmatching_cost(2.0, 5.0, 2.0, 1e-14))
    rels = [d.to(DEV) for d in c["dense"]]
    ptrs = torch.tensor([r.data_ptr() for r in rels], dtype=torch.int64).to(DEV)
    bits = T.pack_relations([{"rel_triplets": t} for t in c["trips"]], c["N"], c["R"], DEV)
    results = {}
    for packed, target in ((False, ptrs), (True, bits)):
        runs = []
        for _ in range(5):
            out = ops.relation_loss_launch(pr, pc, target, packed, pi, ti, mc, off, nm, K_TIE, K_TIE, deterministic=True)
            torch.cuda.synchronize()
            runs.append([t.cpu() for t in out])
        for r in runs[1:]:
            for a, b in zip(runs[0], r):
                assert RT.same_bits(a, b)
        loss, grad_rel, grad_conn = runs[0]
        assert np.array_equal(grad_rel.numpy() != 0, mult > 0)
        assert np.abs(grad_rel.double().numpy() - want_grad).max() < 1e-6
        print("loss", float(loss[0]), want_loss)
        assert abs(float(loss[0]) - want_loss) < 1e-6 * abs(want_loss)
        results[packed] = runs[0]
    for a, b in zip(results[False], results[True]):
        assert RT.same_bits(a, b)
    # the switch reaches the kernels through the autograd Function as well
    with ops.deterministic():
        prg = pr.clone().requires_grad_(True)
        l_rel, l_conn = ops.RelationLossFunction.apply(prg, pc, bits, pi, ti, mc, off, nm, ("largest", K_TIE), ("largest", K_TIE), 0, 0,
                                                       True)
        l_rel.backward()
    assert RT.same_bits(prg.grad.cpu(), results[True][1])


# ------------------------------------------------------------------------------------------------------------ gate means
@pytest.mark.parametrize("train", [False, True])
def test_gate_means_are_reproducible(train):
    import test_gpu_kernels as GK
    from egtr_amd import ops
    d, trip, node = GK._head_inputs(84, 2, 24, 4, 7, 11)
    dd = {k: v.to(DEV).requires_grad_(train) for k, v in d.items()}
    args = (*dd.values(), trip.to(DEV), node.to(DEV), True)
    with torch.set_grad_enabled(train):
        rel0, conn0, gm0 = ops.relation_head(*args)
        with ops.deterministic():
            a = ops.relation_head(*args)
            b = ops.relation_head(*args)
    assert a[2] is not None and tuple(a[2].shape) == (4,)
    assert torch.equal(a[2], b[2])
    assert (a[2] - gm0).abs().max() < 1e-6
    assert torch.equal(a[0], rel0) and torch.equal(a[1], conn0)     # the outputs never depended on the gate-mean buffer


# --------------------------------------------------------------------------------------------------------- model segment
@pytest.fixture(scope="module")
def small(golden_dir):
    import json
    g = Hh.load_golden(golden_dir, "sgg_small.npz")
    return g, json.loads(str(g["cfg"])), json.loads(str(g["shapes"]))


class _Sources(torch.nn.Module):
    """The captured outputs of the input-projection modules as parameters, so that a graphed step returns their gradients."""

    def __init__(self, captured):
        super().__init__()
        self.src = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in captured])


def _segment_run(base, captured, batch, graph, seed):
    from egtr_amd.runtime import DataParallelTrainer, configure_optimizers
    model = copy.deepcopy(base)
    proj = model.model.input_proj
    for p in list(model.model.backbone.parameters()) + list(proj.parameters()):
        p.requires_grad_(False)               # nothing in front of the captured sources takes part in the step
    opt = configure_optimizers(model, lr=1e-4, lr_backbone=1e-5, lr_initialized=None, weight_decay=1e-4)
    model.captured_sources = _Sources(captured)
    for l, m in enumerate(proj):
        m.register_forward_hook(lambda mod, inp, out, l=l: model.captured_sources.src[l])
    torch.manual_seed(seed)
    # accumulate = 2 and ONE micro-step: forward + backward without the optimizer step that would clear the gradients
    tr = DataParallelTrainer(model, optimizer=opt, accumulate=2, clip=0.1, graph=graph, deterministic=True)
    loss, loss_dict, stepped = tr.training_step(batch)
    torch.cuda.synchronize()
    assert not stepped and (tr._graphed is not None) == graph
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()
             if p.grad is not None and (".encoder.layers." in n or ".decoder.layers." in n or "captured_sources" in n)}
    return loss.detach().clone(), {k: v.detach().clone() for k, v in loss_dict.items()}, grads


@pytest.mark.parametrize("graph", [False, True])
def test_model_segment_is_bit_reproducible(small, graph):
    """Encoder, decoder, heads and losses of the small model with dropout 0.1, forward and backward, twice from deep copies and
    the same seed under DataParallelTrainer(deterministic=True): total loss, every loss_dict entry, the gradients of every
    encoder-layer / decoder-layer parameter and the gradients with respect to the input-projection outputs are bit-equal.  The
    input-projection outputs are captured once and returned from forward hooks, so no vendor convolution feeds the segment."""
    from egtr_amd import ops
    g, cfg_dict, shapes = small
    cfg_dict = dict(cfg_dict, dropout=0.1)
    base, cfg, sd = Hh.build_product_model(cfg_dict, shapes, int(g["seed"]))
    base.load_state_dict(sd)
    base = base.to(DEV).train()
    targets = [{k: t.to(DEV) for k, t in d.items()}
               for d in W.make_targets(5, 2, cfg.num_queries, cfg.num_labels, cfg.num_rel_labels)]
    pv, pm = Hh.small_inputs(g)
    batch = {"pixel_values": pv.to(DEV), "pixel_mask": pm.to(DEV), "labels": targets}
    captured = [None] * len(base.model.input_proj)
    handles = [m.register_forward_hook(lambda mod, inp, out, l=l: captured.__setitem__(l, out.detach().clone()))
               for l, m in enumerate(base.model.input_proj)]
    base(pixel_values=batch["pixel_values"], pixel_mask=batch["pixel_mask"], labels=targets, output_attention_states=True)
    for h in handles:
        h.remove()
    assert all(t is not None for t in captured)
    was, vendor_was = ops.DETERMINISTIC, torch.backends.cudnn.deterministic
    try:
        (l0, d0, g0), (l1, d1, g1) = (_segment_run(base, captured, batch, graph, 1234) for _ in range(2))
        assert torch.backends.cudnn.deterministic is True      # requested of the vendor library by the trainer
    finally:
        torch.backends.cudnn.deterministic = vendor_was        # process-wide: not left behind for the tests that follow
    assert ops.DETERMINISTIC == was
    assert torch.isfinite(l0) and torch.equal(l0, l1)
    assert set(d0) == set(d1) and any(k.startswith("rel_gate_") for k in d0)
    for k in d0:
        assert torch.equal(torch.as_tensor(d0[k]), torch.as_tensor(d1[k])), k
    n_layer = sum(1 for n, p in base.named_parameters() if ".encoder.layers." in n or ".decoder.layers." in n)
    assert len(g0) == n_layer + len(captured) and set(g0) == set(g1)
    for n in g0:
        assert float(g0[n].abs().max()) > 0 or "captured" not in n, n
        assert torch.equal(g0[n], g1[n]), n
