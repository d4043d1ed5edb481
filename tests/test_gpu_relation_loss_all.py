"""GPU (-m gpu): the un-sampled relation loss (csrc/loss.hip: rel_all_prep, rel_loss_all, conn_loss, rel_loss_all_finalize; the
C entries egtr_relation_loss_all_f32 on dense and packed targets) against the float64 restatement of tests/relation_loss_all_restated.py (pinned
to the criterion's own composition, and its wrong neighbours shown to move, by tests/test_relation_loss_all_cpu.py), its
bit-level properties, its value-only launch, and the routes that lead to it: the criterion in evaluation mode and in the
un-sampled training configuration, ``DataParallelTrainer.validation_step``.

Bars: losses 1e-5 relative (RA.LOSS_BAR: the training kernel's bar); gradients 8 * 2^-24 / count per element (RA.grad_bar: eight
fp32 roundings of a value of magnitude <= 1 times the count reciprocal).  Every test prints the largest ratio it saw (-s).
Largest seen on an MI355X: gradients 0.28 of their bar (N = 1030), losses 5e-8 relative."""
import json

import numpy as np
import pytest
import torch

import helpers as Hh
import relation_loss_all_restated as RA
import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def flat(c):
    return RA.matcher_flat(c["indices"], c["costs"], DEV)


def launch(c, packed, want_grad=True, nm_cost=RA.NM_COST):
    """ops.relation_loss_all_launch on a case -> (loss [2], grad_rel, grad_conn) on the host (gradients None when not asked for)"""
    from egtr_amd import ops, targets as T
    pr, pc = c["pred_rel"].to(DEV), c["pred_conn"].to(DEV)
    pi, ti, mc, off = flat(c)
    if packed:
        target = keep = T.pack_relations([{"rel_triplets": t} for t in c["trips"]], c["N"], c["R"], DEV)
    else:
        keep = [d.contiguous().to(DEV) for d in c["dense"]]
        target = torch.tensor([r.data_ptr() for r in keep], dtype=torch.int64).to(DEV)
    out = ops.relation_loss_all_launch(pr, pc, target, packed, pi, ti, mc, off, nm_cost, want_grad=want_grad)
    torch.cuda.synchronize()
    del keep
    return [None if t is None else t.cpu() for t in out]


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def close_or_same_nonfinite(got, want, bar_rel):
    """a loss value: the same non-finite value, or within ``bar_rel`` relative; returns the error as a fraction of the bar"""
    if not np.isfinite(want):
        assert (np.isnan(want) and np.isnan(got)) or got == want, (got, want)
        return 0.0
    err = abs(got - want) / abs(want)
    assert err <= bar_rel, (got, want, err)
    return err / bar_rel


FORMS = [(n, False) for n in RA.case_names()] + [(n, True) for n in RA.case_names(packed=True)]


@pytest.mark.parametrize("logits,nm_cost", [("finite", RA.NM_COST), ("nonfinite", RA.NM_COST), ("finite", RA.NM_HALF)])
@pytest.mark.parametrize("name,packed", FORMS)
def test_kernel_vs_float64_restatement(name, packed, logits, nm_cost):
    """Every case under the criterion's non-matching cost, and once more with a cost of 0 (an unmatched query weighs 1 / 2
    instead of 0): there the target rows of unmatched queries and their weight show in y (RA.TEETH, test_relation_loss_all_cpu)."""
    c = RA.case(name, logits)
    loss, g_rel, g_conn = launch(c, packed, nm_cost=nm_cost)
    l_rel, l_conn, r_rel, r_conn = RA.restate(c["pred_rel"], c["pred_conn"], c["dense"], c["indices"], c["costs"], nm_cost)
    if logits == "finite":
        assert np.isfinite(l_rel) and np.isfinite(r_rel).all()
    else:
        assert not np.isfinite(l_rel)        # a NaN logit: NaN, as in the reference
    ratio = [close_or_same_nonfinite(float(loss[0]), l_rel, RA.LOSS_BAR), close_or_same_nonfinite(float(loss[1]), l_conn, RA.LOSS_BAR)]
    for g, r in ((g_rel.double().numpy(), r_rel), (g_conn.double().numpy(), r_conn)):
        fin = np.isfinite(r)
        assert np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(g[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)])
        ratio.append(float(np.abs(g[fin] - r[fin]).max()) / RA.grad_bar(r.size))
    print(f"{name} packed={packed} {logits} nm_cost={nm_cost:.1f}: error / bar -- loss_rel {ratio[0]:.3f}, loss_conn {ratio[1]:.3f}, "
          f"grad_rel {ratio[2]:.3f}, grad_conn {ratio[3]:.3f}")
    assert ratio[2] <= 1.0 and ratio[3] <= 1.0


@pytest.mark.parametrize("packed", [False, True])
def test_sparse_targets_at_fifty_predicates(packed):
    """~20 triplets per image at R = 50: most pair flags stay 0, so the connectivity comparison sees every flag ``rel_loss_all``
    writes or leaves (with the 30 % targets of the other cases every pair is flagged)."""
    c = RA.case("n9r50", "finite", False, True)
    loss, g_rel, g_conn = launch(c, packed)
    l_rel, l_conn, r_rel, r_conn = RA.restate(c["pred_rel"], c["pred_conn"], c["dense"], c["indices"], c["costs"])
    ratio = (close_or_same_nonfinite(float(loss[0]), l_rel, RA.LOSS_BAR), close_or_same_nonfinite(float(loss[1]), l_conn, RA.LOSS_BAR),
             float(np.abs(g_rel.double().numpy() - r_rel).max()) / RA.grad_bar(r_rel.size),
             float(np.abs(g_conn.double().numpy() - r_conn).max()) / RA.grad_bar(r_conn.size))
    print("n9r50 sparse packed=%s: error / bar -- loss_rel %.3f, loss_conn %.3f, grad_rel %.3f, grad_conn %.3f" % ((packed,) + ratio))
    assert ratio[2] <= 1.0 and ratio[3] <= 1.0


def test_nonbinary_dense_targets_are_numbers_in_y_and_flags_in_the_connectivity():
    c = RA.case("n9r50", "finite", True)
    loss, g_rel, g_conn = launch(c, False)
    l_rel, l_conn, r_rel, r_conn = RA.restate(c["pred_rel"], c["pred_conn"], c["dense"], c["indices"], c["costs"])
    ratio = (close_or_same_nonfinite(float(loss[0]), l_rel, RA.LOSS_BAR), close_or_same_nonfinite(float(loss[1]), l_conn, RA.LOSS_BAR),
             float(np.abs(g_rel.double().numpy() - r_rel).max()) / RA.grad_bar(r_rel.size),
             float(np.abs(g_conn.double().numpy() - r_conn).max()) / RA.grad_bar(r_conn.size))
    print("n9r50 non-binary: error / bar -- loss_rel %.3f, loss_conn %.3f, grad_rel %.3f, grad_conn %.3f" % ratio)
    assert ratio[2] <= 1.0 and ratio[3] <= 1.0
    binary = RA.restate(c["pred_rel"], c["pred_conn"], RA.case("n9r50")["dense"], c["indices"], c["costs"])
    # the 0.5 / 2.0 are felt, and in y only: read as 0 / 1 flags they would move gradient elements by far more than the bar
    assert np.abs(binary[2] - r_rel).max() > 1e4 * RA.grad_bar(r_rel.size) and binary[1] == l_conn
    assert np.array_equal(binary[3], r_conn)


@pytest.mark.parametrize("name", RA.case_names(packed=True))
def test_dense_and_packed_entries_give_the_same_bits_run_after_run(name):
    c = RA.case(name)
    d, p, d2 = launch(c, False), launch(c, True), launch(c, False)
    for a, b, e, what in zip(d, p, d2, ("loss_out", "grad_rel", "grad_conn")):
        assert same_bits(a, b), what
        assert same_bits(a, e), what


def test_more_than_64_predicates_is_the_dense_entry_alone():
    from egtr_amd import _lib, ops, targets as T
    c = RA.case("n6r65")
    with pytest.raises(ValueError, match="at most 64"):
        T.pack_relations([{"rel_triplets": t} for t in c["trips"]], c["N"], c["R"], DEV)
    pi, ti, mc, off = flat(c)
    words = torch.zeros(c["B"], c["N"], c["N"], dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.EgtrHipError, match="status -3"):
        ops.relation_loss_all_launch(c["pred_rel"].to(DEV), c["pred_conn"].to(DEV), words, True, pi, ti, mc, off, RA.NM_COST)


def test_refused_image_counts_as_an_image_without_matches():
    """-1 indices (a cost matrix the matcher refused): T = 0 for that image, never an out-of-bounds access."""
    c = RA.case("n9r50")
    a0, b0 = c["indices"][0]
    minus = dict(c, indices=[(torch.full_like(a0, -1), torch.full_like(b0, -1))] + list(c["indices"][1:]))
    none = dict(c, indices=[(a0[:0], b0[:0])] + list(c["indices"][1:]), costs=[c["costs"][0][:0]] + list(c["costs"][1:]))
    got = launch(dict(minus, costs=c["costs"]), True)
    want = launch(none, True)
    for a, b, what in zip(got, want, ("loss_out", "grad_rel", "grad_conn")):
        assert same_bits(a, b), what
    l_rel = RA.restate(c["pred_rel"], c["pred_conn"], c["dense"], minus["indices"], c["costs"])[0]
    assert abs(float(got[0][0]) - l_rel) <= RA.LOSS_BAR * abs(l_rel)


def wide_case():
    """the (3, 9, 50) case scaled to N = 64: 2.4 MB of logits"""
    rng = np.random.default_rng(5200)
    B, N, R = 3, 64, 50
    images = [(rng.permutation(N)[:T], rng.permutation(T), np.argwhere(rng.random((N, N, R)) < 0.05)) for T in (4, 0, 9)]
    import loss_restated as LR
    return LR.build_case(rng, rng.standard_normal((B, N, N, R)).astype(np.float32), images)


def test_value_only_launch_writes_and_allocates_no_gradient():
    from egtr_amd import ops, targets as T
    c = RA.case("n9r50")
    for packed in (False, True):
        full, value = launch(c, packed), launch(c, packed, want_grad=False)
        assert value[1] is None and value[2] is None and same_bits(full[0], value[0])
    # a sentinel-filled buffer of the gradient's size, handed to nobody, next to the launch's own allocations
    c = wide_case()
    B, N, R = c["B"], c["N"], c["R"]
    pr, pc = c["pred_rel"].to(DEV), c["pred_conn"].to(DEV)
    pi, ti, mc, off = flat(c)
    bits = T.pack_relations([{"rel_triplets": t} for t in c["trips"]], N, R, DEV)
    sentinel = torch.full((B, N, N, R), -7.25, device=DEV)
    want = ops.relation_loss_all_launch(pr, pc, bits, True, pi, ti, mc, off, RA.NM_COST)[0].clone()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    with torch.no_grad():
        l_rel, l_conn = ops.RelationLossAllFunction.apply(pr, pc, bits, pi, ti, mc, off, RA.NM_COST, True)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"value-only call: peak grows by {grown} bytes; one gradient would be {B * N * N * R * 4}")
    assert grown < B * N * N * R * 4
    assert same_bits(torch.stack([l_rel, l_conn]).cpu(), want.cpu())
    assert bool((sentinel == -7.25).all())
    # ... and with inputs that require grad the gradients exist, and scale in the backward
    prg, pcg = pr.clone().requires_grad_(True), pc.clone().requires_grad_(True)
    l_rel, l_conn = ops.RelationLossAllFunction.apply(prg, pcg, bits, pi, ti, mc, off, RA.NM_COST, True)
    (3.0 * l_rel + 0.5 * l_conn).backward()
    _, g_rel, g_conn = ops.relation_loss_all_launch(pr, pc, bits, True, pi, ti, mc, off, RA.NM_COST)
    assert torch.equal(prg.grad, g_rel * 3.0) and torch.equal(pcg.grad, g_conn * 0.5)


def test_relation_losses_under_the_deterministic_mode_gives_the_same_bits():
    from egtr_amd import ops
    c = RA.case("n9r50")
    pr, pc = c["pred_rel"].to(DEV), c["pred_conn"].to(DEV)
    idx = [(a.to(DEV), b.to(DEV)) for a, b in c["indices"]]
    costs = [x.to(DEV) for x in c["costs"]]
    res = {}
    for form, tg in (("dense", [{"rel": d.to(DEV)} for d in c["dense"]]), ("trip", [{"rel_triplets": t} for t in c["trips"]])):
        for det in (False, True):
            with ops.deterministic(det):
                prg = pr.clone().requires_grad_(True)
                l_rel, l_conn = ops.relation_losses(prg, pc, tg, idx, costs, RA.NM_COST, None, None)
                g, = torch.autograd.grad(l_rel, prg)
            res[form, det] = (torch.stack([l_rel.detach(), l_conn.detach()]).cpu(), g.cpu())
    for k in res:
        assert same_bits(res[k][0], res["dense", False][0]) and same_bits(res[k][1], res["dense", False][1]), k


# ---------------------------------------------------------------------------------------------------------------- criterion
def criterion(N, R, model_training):
    return RA.criterion(N, R, model_training).to(DEV)


def test_unsampled_training_configuration_gradient_switch_on_vs_off(monkeypatch):
    """``rel_sample_* = None`` in training mode: d loss_rel / d pred_rel from the kernel route and from the tensor composition
    (switch off) differ by no more than the kernel's bar plus the composition's own fp32 error, measured against float64 here."""
    from egtr_amd import ops
    c = RA.case("n9r50")
    crit = criterion(c["N"], c["R"], True)
    tg = [{"rel": d.to(DEV)} for d in c["dense"]]
    idx = [(a.to(DEV), b.to(DEV)) for a, b in c["indices"]]
    costs = [x.to(DEV) for x in c["costs"]]
    got = {}
    for on in (True, False):
        monkeypatch.setattr(ops, "RELATION_LOSS_ALL", on)
        calls = []
        orig = ops.relation_losses
        monkeypatch.setattr(ops, "relation_losses", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
        pr = c["pred_rel"].to(DEV).requires_grad_(True)
        out = crit.loss_relations({"pred_rel": pr, "pred_connectivity": c["pred_conn"].to(DEV)}, tg, idx, costs, 1.0)
        monkeypatch.setattr(ops, "relation_losses", orig)
        assert len(calls) == (1 if on else 0)
        g, = torch.autograd.grad(out["loss_rel"], pr)
        got[on] = (float(out["loss_rel"]), float(out["loss_connectivity"]), g.double().cpu().numpy())
    l_rel, l_conn, r_rel, _ = RA.restate(c["pred_rel"], c["pred_conn"], c["dense"], c["indices"], c["costs"],
                                         nm_cost=float(crit.nonmatching_cost))
    bar = RA.grad_bar(r_rel.size)
    comp_err = float(np.abs(got[False][2] - r_rel).max())
    diff = float(np.abs(got[True][2] - got[False][2]).max())
    print(f"gradient: switch on vs off {diff / bar:.3f} bars, the composition vs float64 {comp_err / bar:.3f} bars, "
          f"the kernel vs float64 {float(np.abs(got[True][2] - r_rel).max()) / bar:.3f} bars")
    assert diff <= bar + comp_err
    for k in (0, 1):
        assert abs(got[True][k] - got[False][k]) <= RA.LOSS_BAR * abs(got[False][k])


@pytest.fixture(scope="module")
def small_model(golden_dir):
    g = Hh.load_golden(golden_dir, "sgg_small.npz")
    cfg_dict, shapes = json.loads(str(g["cfg"])), json.loads(str(g["shapes"]))
    model, cfg, sd = Hh.build_product_model(cfg_dict, shapes, int(g["seed"]))
    model.load_state_dict(sd)
    return g, model.to(DEV), cfg


def _targets(g, cfg):
    host = W.make_targets(int(g["target_seed"]), 2, cfg.num_queries, cfg.num_labels, cfg.num_rel_labels)
    dense = [{k: v.to(DEV) for k, v in t.items()} for t in host]
    trip = [{"class_labels": t["class_labels"].to(DEV), "boxes": t["boxes"].to(DEV), "rel_triplets": t["rel"].nonzero()}
            for t in host]
    return dense, trip


@pytest.mark.parametrize("form", ["dense", "trip"])
def test_evaluation_mode_loss_dict_switch_on_vs_off(small_model, form, monkeypatch):
    """The evaluation-mode criterion on ONE forward of the small model, switch on and off: every term within LOSS_BAR.  With
    triplet targets the new route builds no dense target and calls no ``torch.nonzero``: both raise while the switch is on."""
    from egtr_amd import ops
    from egtr_amd.egtr import SceneGraphGenerationLoss
    g, model, cfg = small_model
    model.eval()
    pv, pm = Hh.small_inputs(g)
    dense, trip = _targets(g, cfg)            # (before ``torch.nonzero`` is made to raise)
    targets = dense if form == "dense" else trip
    seen = {}
    orig_forward = SceneGraphGenerationLoss.forward

    def forbidden(*a, **k):
        raise AssertionError("the un-sampled kernel route builds no dense target and no index list")

    def both(self, outputs, tg, matched=None):
        assert self.model_training is False
        with monkeypatch.context() as m:
            m.setattr(ops, "RELATION_LOSS_ALL", False)
            seen["off"] = dict(orig_forward(self, outputs, tg, matched))
        with monkeypatch.context() as m:
            if form == "trip":
                m.setattr(SceneGraphGenerationLoss, "_dense_targets", forbidden)
                m.setattr(torch, "nonzero", forbidden)
            on = orig_forward(self, outputs, tg, matched)
        seen["on"] = dict(on)         # (the model adds its own entries to the dict it gets back)
        return on

    monkeypatch.setattr(SceneGraphGenerationLoss, "forward", both)
    with torch.no_grad():
        out = model(pixel_values=pv.to(DEV), pixel_mask=pm.to(DEV), labels=targets, output_attentions=False,
                    output_attention_states=True, output_hidden_states=True)
    assert bool(torch.isfinite(out.loss))
    assert set(seen["on"]) == set(seen["off"]) and {"loss_rel", "loss_connectivity"} <= set(seen["on"])
    worst = 0.0
    for k in seen["on"]:
        a, b = float(seen["on"][k]), float(seen["off"][k])
        assert abs(a - b) <= RA.LOSS_BAR * abs(b), (k, a, b)
        worst = max(worst, abs(a - b) / (abs(b) or 1.0) / RA.LOSS_BAR)
    print(f"evaluation mode, {form} targets: worst term differs by {worst:.3f} bars")


def test_validation_step_equals_the_evaluation_mode_forward(small_model, monkeypatch):
    """``validation_step`` returns the loss of the evaluation-mode forward it runs, bit for bit -- compared with THAT forward (the
    model's ``forward`` is recorded).  A second, separately run evaluation-mode forward is held to LOSS_BAR: two forwards of this
    project's model are not bit-reproducible run to run (MIOpen's convolutions; tests/test_gpu_rel_targets.py,
    test_training_step_with_triplet_targets_equals_dense_targets).  The matcher statuses of the validation forward do not stay
    behind, and the ones of the accumulation window in flight do."""
    from egtr_amd.runtime import DataParallelTrainer
    g, model, cfg = small_model
    pv, pm = Hh.small_inputs(g)
    _, trip = _targets(g, cfg)
    batch = {"pixel_values": pv.to(DEV), "pixel_mask": pm.to(DEV), "labels": trip}
    model.train()
    tr = DataParallelTrainer(model, optimizer=torch.optim.SGD(model.parameters(), lr=0.0), accumulate=1)
    seen = []
    orig = type(model).forward

    def recorded(self, *a, **k):
        out = orig(self, *a, **k)
        seen.append((self.training, torch.is_grad_enabled(), out.loss.clone(), {n: v.clone() for n, v in out.loss_dict.items()}))
        return out

    import egtr_amd.deformable_detr as dd
    dd.DeformableDetrHungarianMatcher.take_step_statuses()
    window = torch.zeros(2, dtype=torch.int32, device=DEV)
    dd._STEP_MATCHER_STATUS.append(window)
    with monkeypatch.context() as m:
        m.setattr(type(model), "forward", recorded)
        loss, d = tr.validation_step(batch)
    left = dd.DeformableDetrHungarianMatcher.take_step_statuses()
    assert len(left) == 1 and left[0] is window
    assert len(seen) == 1 and seen[0][:2] == (False, False)               # one forward, evaluation mode, no autograd graph
    assert model.training and not loss.requires_grad and d["loss"] is loss
    assert all(p.grad is None for p in model.parameters())
    assert set(d) == set(seen[0][3]) | {"loss"} and {"loss_rel", "loss_connectivity"} <= set(d)
    assert same_bits(loss.reshape(1).cpu(), seen[0][2].reshape(1).cpu())
    for k, v in seen[0][3].items():
        assert same_bits(d[k].reshape(1).float().cpu(), v.reshape(1).float().cpu()), k
    model.eval()
    with torch.no_grad():
        out = model(pixel_values=batch["pixel_values"], pixel_mask=batch["pixel_mask"], labels=trip, output_attentions=False,
                    output_attention_states=True, output_hidden_states=True)
    assert set(d) == set(out.loss_dict) | {"loss"}
    err = abs(float(loss) - float(out.loss)) / abs(float(out.loss))
    print(f"validation_step against a separately run evaluation-mode forward: {err:.3e} relative")
    assert err <= RA.LOSS_BAR
    summary = DataParallelTrainer.validation_epoch_end([(loss, d), (loss, d)])
    assert summary["validation_loss"] == float(loss) and summary["validation_loss_rel"] == float(d["loss_rel"])
