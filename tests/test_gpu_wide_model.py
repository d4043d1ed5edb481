"""GPU (-m gpu): the product model with num_rel_labels = 100 on the HIP kernels against the reference's own run,
tests/golden/sgg_small_wide.npz (tests/golden/make_golden_wide.py).  Inference takes egtr_rel_head_forward_wide_bf16x6_f32,
training egtr_rel_head_forward_wide_f32; before these entries existed the first forward ended in status -3.  Tolerances: those of
test_gpu_model.py::test_two_stage_model_vs_reference.  The CPU twin is tests/test_wide_model_cpu.py."""
import pytest
import torch

import helpers as Hh
import wide_model_cases as WM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(out=1e-3, loss=1e-3, grad=5e-3, grad_floor=1e-2)


@pytest.fixture
def wide(golden_dir):
    return WM.load(golden_dir, DEV)


def test_wide_model_eval_forward_vs_reference(wide, monkeypatch):
    from egtr_amd import _lib, ops
    g, model, cfg, pv, pm = wide
    names = []
    real_launch = _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda name, *a, **k: (names.append(name), real_launch(name, *a, **k))[1])
    before = dict(ops.FALLBACKS)
    WM.check_eval_forward(g, model, pv, pm, TOL["out"])
    assert "egtr_rel_head_forward_wide_bf16x6_f32" in names and names.count("egtr_rel_head_streams_wide_f32") == 1
    WM.check_logit_adjustment(g, model, pv, pm, TOL["out"])
    assert ops.FALLBACKS == before


def test_wide_model_bf16_forward_vs_its_own_fp32_forward(wide):
    """The bf16 model has no fast relation head above 64 predicates: the fp32 wide kernel runs on widened operands and the outputs
    are cast back.  (max, mean) errors of the O(1) quantities under the only bf16 model tolerance test_gpu_model.py states,
    test_stress_geometry_bf16_vs_reference_with_bf16_weights: class logits (0.27, 0.022), boxes (0.016, 0.003), connectivity and
    relation-MLP logits (0.22, 0.021); frequency bias off, as there (a bf16 tensor cannot hold -29 + x)."""
    g, model, cfg, pv, pm = wide
    model.config.use_freq_bias = False
    ref = Hh.product_heads(model, pv, pm)
    ref = {k: v.float().cpu() for k, v in ref.items()}
    model = model.to(torch.bfloat16)
    got = Hh.product_heads(model, pv.to(torch.bfloat16), pm)
    assert got["rel_logits"].dtype == torch.bfloat16 and tuple(got["rel_logits"].shape) == (2, 24, 24, 100)
    tols = {"logits": (0.27, 0.022), "pred_boxes": (0.016, 0.003), "conn_logits": (0.22, 0.021), "rel_logits": (0.22, 0.021)}
    errs = {}
    for key, (mx, mean) in tols.items():
        d = (got[key].float().cpu() - ref[key]).abs()
        errs[key] = (float(d.max()), float(d.mean()))
    print("bf16 wide model against its fp32 forward (max, mean):", errs)
    for key, (mx, mean) in tols.items():
        assert errs[key][0] < mx and errs[key][1] < mean, (key, errs)


def test_wide_model_train_step_vs_reference_with_dense_and_triplet_targets(wide):
    from egtr_amd import ops
    g, model, cfg, pv, pm = wide
    before = dict(ops.FALLBACKS)
    WM.check_train_step(g, model, cfg, pv, pm, TOL)
    WM.check_train_step(g, model, cfg, pv, pm, TOL, triplets=True)
    # (two whole steps are not comparable bit for bit here: MIOpen's convolutions are not reproducible run to run)
    WM.check_loss_equal_between_target_forms(g, model, cfg, pv, pm, TOL)
    with ops.deterministic():
        WM.check_loss_equal_between_target_forms(g, model, cfg, pv, pm, TOL)
    assert ops.FALLBACKS == before


def test_wide_model_validation_step_vs_reference(wide):
    g, model, cfg, pv, pm = wide
    WM.check_validation_step(g, model, cfg, pv, pm, TOL, bitwise_forms=False)


def test_wide_model_evaluate_and_graph_replay(wide):
    """evaluate() through a captured graph returns finite recalls, and a strict GraphedForward of the R = 100 model captures and
    replays equal to the eager forward: nothing in the wide route allocates or synchronises at capture time.  "Equal": to 1e-5,
    the bar of test_gpu_model.py::test_graph_replay_follows_weight_updates (MIOpen's convolutions are not bit-reproducible)."""
    from egtr_amd.runtime import GraphedForward
    g, model, cfg, pv, pm = wide
    WM.check_evaluate(model, cfg, pv, pm, graphed=True)
    with torch.no_grad():
        eager = model(pixel_values=pv, pixel_mask=pm, output_attention_states=True, output_hidden_states=True)
        fwd = GraphedForward(model, strict=True)
        fwd(pv, pm)
        out = fwd(pv, pm)
    assert fwd.graphed
    for k in ("logits", "pred_boxes", "pred_rel", "pred_connectivity"):
        assert float((out[k] - eager[k]).abs().max()) < 1e-5, k
