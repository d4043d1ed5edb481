"""The model-level checks of a 100-predicate model against the reference's own run (tests/golden/sgg_small_wide.npz, written by
tests/golden/make_golden_wide.py), shared by tests/test_wide_model_cpu.py (CPU stand-ins) and tests/test_gpu_wide_model.py (HIP
kernels).  ``tol``: dict(out, loss, grad, grad_floor) -- the tolerances of the two existing two-stage tests, which the callers
take over: test_host_model_cpu.py::test_two_stage_model_matches_reference (2e-4, 3e-4, 2e-3 with floor 1e-3) and
test_gpu_model.py::test_two_stage_model_vs_reference (1e-3, 1e-3, 5e-3 with floor 1e-2)."""
import json

import torch

import helpers as Hh
import weights as W


def _t(a):
    return torch.from_numpy(a)


def load(golden_dir, dev):
    g = Hh.load_golden(golden_dir, "sgg_small_wide.npz")
    cfg_dict, shapes = json.loads(str(g["cfg"])), json.loads(str(g["shapes"]))
    assert cfg_dict["num_rel_labels"] == 100 and cfg_dict["auxiliary_loss"] and cfg_dict["use_freq_bias"]
    model, cfg, sd = Hh.build_product_model(cfg_dict, shapes, int(g["seed"]))
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    pv, pm = Hh.small_inputs(g)
    return g, model, cfg, pv.to(dev), pm.to(dev)


def targets_of(g, cfg, dev, triplets=False):
    out = []
    for t in W.make_targets(int(g["target_seed"]), 2, cfg.num_queries, cfg.num_labels, cfg.num_rel_labels):
        t = {k: v.to(dev) for k, v in t.items()}
        if triplets:
            t["rel_triplets"] = t.pop("rel").nonzero()
        out.append(t)
    return out


def check_eval_forward(g, model, pv, pm, tol):
    h = Hh.product_heads(model, pv, pm)
    assert tuple(h["rel_logits"].shape) == (2, 24, 24, 100)
    assert (h["logits"].cpu() - _t(g["logits"])).abs().max() < tol and (h["pred_boxes"].cpu() - _t(g["pred_boxes"])).abs().max() < tol
    rel_mlp = Hh.rel_mlp_from_logits(h["rel_logits"].cpu(), h["logits"].cpu(), model.triplet_dist.cpu())
    assert (rel_mlp - _t(g["rel_mlp"])).abs().max() < tol
    assert (h["conn_logits"].cpu() - _t(g["conn_logits"])).abs().max() < tol
    with torch.no_grad():
        out = model(pixel_values=pv, pixel_mask=pm)
    assert (out.pred_rel[..., -1].cpu() - _t(g["pred_rel_last"])).abs().max() < tol
    assert (out.pred_rel.cpu() - torch.sigmoid(h["rel_logits"].cpu())).abs().max() < 1e-6
    return out


def check_logit_adjustment(g, model, pv, pm, tol):
    model.config.logit_adjustment = True
    try:
        with torch.no_grad():
            out = model(pixel_values=pv, pixel_mask=pm)
    finally:
        model.config.logit_adjustment = False
    assert (out.pred_rel[:, ::2].cpu() - _t(g["pred_rel_adjusted"])).abs().max() < tol


def _train_step(model, pv, pm, targets):
    model.train()
    model.zero_grad(set_to_none=True)
    out = model(pixel_values=pv, pixel_mask=pm, labels=targets, output_attention_states=True)
    out.loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    model.eval()
    return out, grads


def check_train_step(g, model, cfg, pv, pm, tol, triplets=False):
    """one train step against the reference's loss dict, total loss and every gradient norm"""
    dev = pv.device
    out_d, grads_d = _train_step(model, pv, pm, targets_of(g, cfg, dev, triplets=triplets))
    ref = json.loads(str(g["train_loss_dict"]))
    assert set(ref) == set(out_d.loss_dict), sorted(set(ref) ^ set(out_d.loss_dict))
    for k, v in ref.items():
        assert abs(float(out_d.loss_dict[k]) - v) < tol["loss"] * max(1.0, abs(v)), (k, float(out_d.loss_dict[k]), v)
    assert abs(float(out_d.loss) - float(g["train_loss"])) < tol["loss"] * abs(float(g["train_loss"]))
    gn = json.loads(str(g["grad_norms"]))
    assert set(gn) == set(grads_d)
    for n, v in gn.items():
        got = float(grads_d[n].norm())
        assert abs(got - v) < tol["grad"] * max(abs(v), tol["grad_floor"]), (n, got, v)
    return out_d, grads_d


def check_full_steps_equal_between_target_forms(g, model, cfg, pv, pm):
    """two whole train steps, dense and triplet-list targets: the same loss dict and gradients bit for bit.  For a model whose
    forward and backward are reproducible run to run (the CPU stand-ins); on the GPU MIOpen's convolutions are not, and
    ``check_loss_equal_between_target_forms`` compares the two forms on ONE forward's tensors."""
    dev = pv.device
    out_d, grads_d = _train_step(model, pv, pm, targets_of(g, cfg, dev))
    out_t, grads_t = _train_step(model, pv, pm, targets_of(g, cfg, dev, triplets=True))
    assert set(out_t.loss_dict) == set(out_d.loss_dict) and set(grads_t) == set(grads_d)
    for k in out_d.loss_dict:
        assert torch.equal(out_t.loss_dict[k], out_d.loss_dict[k]), k
    assert torch.equal(out_t.loss, out_d.loss)
    for n in grads_d:
        assert torch.equal(grads_t[n], grads_d[n]), n


def check_loss_equal_between_target_forms(g, model, cfg, pv, pm, tol):
    """the training loss of ONE forward's head outputs with dense and with triplet-list targets: the same loss dict and the same
    gradient of every head output, bit for bit; the triplet form is also held against the reference's loss dict"""
    dev = pv.device
    model.train()
    with torch.no_grad():
        tensors = model.forward_tensors(pv, pm)
    res = {}
    for form in (False, True):
        leaves = [t.detach().clone().requires_grad_(True) if torch.is_tensor(t) and t.is_floating_point() else t
                  for t in tensors]
        loss, loss_dict = model.loss_from_tensors(leaves, targets_of(g, cfg, dev, triplets=form))
        loss.backward()
        res[form] = (loss.detach(), {k: v.detach() for k, v in loss_dict.items()},
                     [t.grad for t in leaves if torch.is_tensor(t) and t.requires_grad])
    model.eval()
    ref = json.loads(str(g["train_loss_dict"]))
    assert set(ref) == set(res[True][1])
    for k, v in ref.items():
        assert abs(float(res[True][1][k]) - v) < tol["loss"] * max(1.0, abs(v)), (k, float(res[True][1][k]), v)
    assert torch.equal(res[False][0], res[True][0])
    for k in res[False][1]:
        assert torch.equal(res[False][1][k], res[True][1][k]), k
    assert len(res[False][2]) == len(res[True][2]) >= 4
    for a, b in zip(res[False][2], res[True][2]):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    assert res[True][2][2] is not None and float(res[True][2][2].abs().sum()) > 0      # pred_rel takes a gradient


def check_validation_step(g, model, cfg, pv, pm, tol, bitwise_forms=True):
    """the un-sampled (evaluation-mode) loss through DataParallelTrainer.validation_step, both target forms (``bitwise_forms``:
    the two runs' loss dicts are equal bit for bit -- where two forwards are reproducible)"""
    from egtr_amd.runtime import DataParallelTrainer
    tr = DataParallelTrainer(model, optimizer=torch.optim.SGD(model.parameters(), lr=0.0), accumulate=1)
    ref = json.loads(str(g["eval_loss_dict"]))
    got = {}
    for form in (False, True):
        batch = {"pixel_values": pv, "pixel_mask": pm, "labels": targets_of(g, cfg, pv.device, triplets=form)}
        loss, d = tr.validation_step(batch)
        assert set(ref) | {"loss"} == set(d), sorted(set(ref) ^ set(d))
        for k, v in ref.items():
            assert abs(float(d[k]) - v) < tol["loss"] * max(1.0, abs(v)), (k, float(d[k]), v)
        assert abs(float(loss) - float(g["eval_loss"])) < tol["loss"] * abs(float(g["eval_loss"]))
        got[form] = d
    for k in got[False]:
        assert not bitwise_forms or torch.equal(got[False][k], got[True][k]), k
    model.eval()


def check_evaluate(model, cfg, pv, pm, graphed):
    """evaluate() on a 100-predicate model runs and returns finite recalls (targets from the model's own predictions)"""
    from egtr_amd.evaluation import evaluate
    C, R = cfg.num_labels, cfg.num_rel_labels
    with torch.no_grad():
        out = model(pixel_values=pv, pixel_mask=pm)
    targets = []
    sizes = torch.tensor([[480, 640], [300, 500]])
    for b in range(2):
        n = 6
        rel = torch.zeros(n, n, R)
        for i in range(n):
            rel[i, (i + 1) % n, 64 + (i * 7) % (R - 64)] = 1
            rel[i, (i + 2) % n, int(out.pred_rel[b, i, (i + 2) % n].argmax())] = 1
        targets.append({"class_labels": out.logits[b, :n, :C].argmax(-1).cpu(), "boxes": out.pred_boxes[b, :n].cpu(), "rel": rel,
                        "orig_size": sizes[b]})
    got = evaluate(model, [{"pixel_values": pv, "pixel_mask": pm, "labels": targets}], C, R, single=True, multiple=True,
                   max_topk=100, graphed=graphed)
    assert got and all(v == v and abs(v) != float("inf") and 0.0 <= v <= 1.0 for v in got.values()), got
    assert got["(single)R@100"] > 0
    return got
