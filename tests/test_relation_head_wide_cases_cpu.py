"""CPU: the host half of tests/test_gpu_relation_head_wide.py -- the relation head above 64 predicate classes
(egtr_rel_head_forward_wide_f32, egtr_rel_head_forward_wide_bf16x6_f32, egtr_rel_head_streams_wide_f32; 1 <= num_rel <= 256).

(1) For every grid case the GPU file launches, what tests/test_relation_head_cases_cpu.py asserts for the narrow grid: float32
evaluation equals float64, every operand and activation is a bf16 number, gates are 0 / 0.5 / 1, both ReLU layers are mixed.
(2) The cases have teeth for THIS change: every output column r >= 32 differs from columns r - 32 and r - 64 in some pair (a kernel
that wraps an output-tile index cannot pass), the last column is more than its bias, a frequency bias varies above column 64.
(3) The three entries validate their arguments before any HIP call.  (4) ``rel_triplets`` targets above 64 predicates are
materialised densely; the packed route still stops at 64."""
import ctypes

import pytest
import torch

import relation_head_restated as RH
from test_relation_head_cases_cpu import _bf16_exact, assert_forward_bits

# (B, N, T, R, C1, sweep), the layout of RH.FORWARD_CASES
WIDE_R_SWEEP = [(2, 9, 7, R, C1, False) for R in (33, 64, 65, 95, 96, 97, 128, 129, 191, 192, 193, 255, 256) for C1 in (0, 5)]
WIDE_N_SWEEP = [(2, N, 7, 100, 12, False) for N in (1, 3, 4, 5, 8, 12, 33)]
WIDE_T_SWEEP = [(2, 9, T, 97, 0, False) for T in range(1, 11)] + [(2, 9, T, 97, 0, True) for T in (7, 9, 10)]
WIDE_CASES = WIDE_R_SWEEP + WIDE_N_SWEEP + WIDE_T_SWEEP
WIDE_ENTRIES = ("egtr_rel_head_forward_wide_f32", "egtr_rel_head_forward_wide_bf16x6_f32", "egtr_rel_head_streams_wide_f32")


@pytest.mark.parametrize("case", WIDE_CASES, ids=RH.case_id)
def test_wide_grid_forward_is_exact_in_float32_and_in_bf16(case):
    B, N, T, R, C1, sweep = case
    d = RH.grid_inputs(RH.case_seed(*case), B, N, T, R, C1, sweep)
    ref = RH.forward(d)
    f32 = RH.forward(d, dtype=torch.float32)
    for name, a, b in zip(("rel", "conn", "gate_mean", "h1", "h2"), f32, ref):
        if name != "gate_mean":
            assert a.dtype == torch.float32 and torch.equal(a, b.float()), name
    assert_forward_bits(f32, ref)
    assert_forward_bits(RH.forward(d, dtype=torch.float32, round_bf16=True), ref, "h1, h2 through bf16: ")
    for k, v in d.items():
        if v.is_floating_point() and not k.startswith("gate_"):
            assert _bf16_exact(v), k
    rel, conn, gm, h1, h2 = (x.float() for x in ref)
    for name, v in (("h1", h1), ("h2", h2), ("rel", rel), ("conn", conn)):
        assert _bf16_exact(v) and float(v.abs().max()) <= 256, (name, float(v.abs().max()))
    if C1:
        assert _bf16_exact(rel - d["triplet"][d["node_cls"][:, :, None], d["node_cls"][:, None, :]])
        assert int(d["node_cls"].min()) == 0 and int(d["node_cls"].max()) == C1 - 1
    g = RH.gates(d["gate_q"], d["gate_k"])
    assert torch.equal(g, RH.gates(d["gate_q"].double(), d["gate_k"].double()).float())
    assert bool(((g == 0) | (g == 0.5) | (g == 1)).all())
    assert float((ref[2] - RH.gate_mean_exact(d["gate_q"], d["gate_k"])).abs().max()) <= 1e-15
    if not sweep:
        for v in (0.0, 0.5, 1.0):
            assert float((g == v).float().mean()) >= 0.10, (v, float((g == v).float().mean()))
    for name, h in (("h1", h1), ("h2", h2)):
        on = float((h > 0).double().mean())
        assert 0.25 <= on <= 0.75, (name, on)


@pytest.mark.parametrize("case", WIDE_CASES, ids=RH.case_id)
def test_wide_grid_cases_tell_the_output_tiles_apart(case):
    B, N, T, R, C1, sweep = case
    d = RH.grid_inputs(RH.case_seed(*case), B, N, T, R, C1, sweep)
    rel = RH.forward(d)[0].reshape(-1, R)                       # float64 [pairs, R]
    for r in range(32, R):
        for back in (32, 64):
            if r - back >= 0:
                assert bool((rel[:, r] != rel[:, r - back]).any()), f"column {r} equals column {r - back} in every pair"
    plain = RH.forward({k: v for k, v in d.items() if k not in ("triplet", "node_cls")})[0].reshape(-1, R)
    assert bool((plain[:, R - 1] != d["b3r"][R - 1].double()).any()), "the last column is its bias alone"
    if C1 and R > 65:
        hi = d["triplet"][:, :, 64:]
        assert bool((hi != hi[:, :, :1]).any()), "the frequency bias is the same in every column above 64"


def test_wide_sweeps_reach_every_instantiation_and_boundary():
    assert {c[2] for c in WIDE_T_SWEEP} == set(range(1, 11))
    rs = {c[3] for c in WIDE_R_SWEEP}
    for edge in (64, 96, 128, 192, 256):
        assert edge in rs and (edge + 1 in rs or edge == 256)
    assert max(rs) == 256 and all(c[3] > 64 for c in WIDE_N_SWEEP + WIDE_T_SWEEP)


# ---- the entries' argument checks come before any HIP call ------------------------------------------------------------------------
def _call(h, name, p, T, hidden, R, trip=None, node=None):
    """one of the three entries with every pointer operand ``p`` (NULL or a host address: never dereferenced on these paths)"""
    if name == "egtr_rel_head_streams_wide_f32":
        return getattr(h, name)(None, p, p, p, hidden, R, p, p, p)
    tail = [trip, node, 1, 5, T, hidden, R, 3, p, p, None]
    extra = [0] if name.endswith("bf16x6_f32") else [None, None]
    return getattr(h, name)(None, *([p] * 13), *tail, *extra)


@pytest.mark.parametrize("name", WIDE_ENTRIES)
def test_wide_entries_validate_their_arguments_without_a_gpu(name):
    from egtr_amd import _lib
    h = _lib.lib()
    E_ARG, E_UNSUPPORTED = -1, -3
    raw = ctypes.create_string_buffer(64 + 16)
    addr = (ctypes.addressof(raw) + 15) & ~15
    assert _call(h, name, None, 7, 256, 100) == E_ARG                       # NULL operands
    assert _call(h, name, addr, 7, 256, 257) == E_UNSUPPORTED               # num_rel past the range
    assert _call(h, name, addr, 7, 128, 100) == E_UNSUPPORTED               # hidden != 256
    assert _call(h, name, addr, 7, 256, 0) == E_ARG
    if name != "egtr_rel_head_streams_wide_f32":
        assert _call(h, name, addr, 10 if name.endswith("bf16x6_f32") else 11, 256, 100) == E_UNSUPPORTED   # slots past the range
        assert _call(h, name, addr, 7, 256, 100, trip=addr, node=None) == E_ARG   # a frequency bias without node_cls
    assert name in _lib.SIGNATURES


# ---- triplet targets above 64 predicates -------------------------------------------------------------------------------------------
def _triplet_targets(N, R):
    g = torch.Generator().manual_seed(31)
    out = []
    for k in (17, 0, 40):
        t = torch.stack([torch.randint(0, N, (k,), generator=g), torch.randint(0, N, (k,), generator=g),
                         torch.randint(0, R, (k,), generator=g)], 1)
        if k:
            t[0, 2], t[1, 2] = R - 1, 64                      # the last predicate and the first one a word cannot hold
            t = torch.cat([t, t[:3]])                         # duplicated rows mean the same as one
        out.append({"rel_triplets": t})
    return out


def _dense_by_hand(t, N, R):
    rel = torch.zeros(N, N, R)
    for s, o, p in t.tolist():
        rel[s, o, p] = 1.0
    return rel


def test_triplet_targets_above_64_predicates_are_materialised_densely():
    from egtr_amd import targets as rt
    N, R = 9, 100
    tg = _triplet_targets(N, R)
    dense = rt.dense_targets(tg, N, R, "cpu")
    for t, d in zip(tg, dense):
        assert d["rel"].dtype == torch.float32 and d["rel"].is_contiguous() and tuple(d["rel"].shape) == (N, N, R)
        assert torch.equal(d["rel"], _dense_by_hand(t["rel_triplets"], N, R))
        assert d["rel_triplets"] is t["rel_triplets"]
    assert float(dense[0]["rel"][..., 64:].sum()) >= 2 and float(dense[1]["rel"].sum()) == 0
    with pytest.raises(ValueError):                                          # host triplets are checked like _check_host
        rt.dense_targets([{"rel_triplets": torch.tensor([[0, 1, R]])}], N, R, "cpu")
    with pytest.raises(ValueError):
        rt.dense_targets([{"rel_triplets": torch.tensor([[0, N, 3]])}], N, R, "cpu")
    with pytest.raises(ValueError):                                          # the packed route still holds 64 predicates
        rt.pack_relations(tg, N, 65, "cpu")
    assert rt.MAX_REL_LABELS == 64


def test_criterion_takes_triplet_targets_at_100_predicates():
    """the criterion's own materialisation (SceneGraphGenerationLoss._dense_targets) equals the dense construction by hand, and
    loss_relations / loss_uncertainty return the same values for the two target forms"""
    from egtr_amd.deformable_detr import DeformableDetrHungarianMatcher
    from egtr_amd.egtr import SceneGraphGenerationLoss
    N, R, C = 9, 100, 5
    g = torch.Generator().manual_seed(7)
    tg = _triplet_targets(N, R)
    for t in tg:
        k = 4
        t["class_labels"] = torch.randint(0, C, (k,), generator=g)
        t["boxes"] = torch.rand(k, 4, generator=g) * 0.5 + 0.25
        t["rel_triplets"] = t["rel_triplets"].clone()
        t["rel_triplets"][:, :2] %= k
    dense_tg = [dict({k: v for k, v in t.items() if k != "rel_triplets"}, rel=_dense_by_hand(t["rel_triplets"], N, R))
                for t in tg]
    matcher = DeformableDetrHungarianMatcher(class_cost=1.0, bbox_cost=5.0, giou_cost=2.0, smoothing=1e-14)
    crit = SceneGraphGenerationLoss(matcher=matcher, num_object_queries=N, num_classes=C, num_rel_labels=R, eos_coef=0.1,
                                    losses=["labels", "boxes", "relations", "uncertainty"], smoothing=1e-14,
                                    rel_sample_negatives=None, rel_sample_nonmatching=None, model_training=True,
                                    focal_alpha=0.25, rel_sample_negatives_largest=True, rel_sample_nonmatching_largest=True)
    for a, b in zip(crit._dense_targets(tg, torch.device("cpu")), dense_tg):
        assert torch.equal(a["rel"], b["rel"])
    B = len(tg)
    outputs = dict(logits=torch.randn(B, N, C, generator=g), pred_boxes=torch.rand(B, N, 4, generator=g) * 0.5 + 0.25,
                   pred_rel=torch.randn(B, N, N, R, generator=g), pred_connectivity=torch.randn(B, N, N, 1, generator=g))
    la, lb = crit(outputs, tg), crit(outputs, dense_tg)
    assert set(la) == set(lb) and {"loss_rel", "loss_connectivity", "uncertainty"} <= set(la)
    for k in la:
        assert torch.equal(la[k], lb[k]), k
