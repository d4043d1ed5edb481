"""CPU (the ``cpu_kernels`` stand-ins for the HIP ops): the product model with num_rel_labels = 100 against the reference's own
run, tests/golden/sgg_small_wide.npz (tests/golden/make_golden_wide.py) -- host logic above 64 predicate classes: the frequency
bias and logit adjustment at R = 100, dense and triplet-list targets through the criterion, the un-sampled validation loss.
Tolerances: those of test_host_model_cpu.py::test_two_stage_model_matches_reference.  The GPU twin is tests/test_gpu_wide_model.py
(it also runs the bf16 model and evaluate(), which need the device kernels)."""
import pytest

import wide_model_cases as WM

TOL = dict(out=2e-4, loss=3e-4, grad=2e-3, grad_floor=1e-3)


@pytest.fixture
def wide(golden_dir, cpu_kernels):
    return WM.load(golden_dir, "cpu")


def test_wide_model_eval_forward_matches_reference(wide):
    g, model, cfg, pv, pm = wide
    WM.check_eval_forward(g, model, pv, pm, TOL["out"])
    WM.check_logit_adjustment(g, model, pv, pm, TOL["out"])


def test_wide_model_train_step_matches_reference_with_dense_and_triplet_targets(wide):
    g, model, cfg, pv, pm = wide
    WM.check_train_step(g, model, cfg, pv, pm, TOL)
    WM.check_train_step(g, model, cfg, pv, pm, TOL, triplets=True)
    WM.check_full_steps_equal_between_target_forms(g, model, cfg, pv, pm)
    WM.check_loss_equal_between_target_forms(g, model, cfg, pv, pm, TOL)


def test_wide_model_validation_step_matches_reference(wide):
    g, model, cfg, pv, pm = wide
    WM.check_validation_step(g, model, cfg, pv, pm, TOL)
