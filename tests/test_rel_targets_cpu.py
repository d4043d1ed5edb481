"""CPU: relation targets as triplet lists (egtr_amd.targets) -- the packed words against the dense tensor
built the reference's way (data/visual_genome.py:74-80), the evaluators' GT entry, the criterion's routes on the small
model, and the two C entries' argument checks."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import helpers as Hh
import weights as W

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import sgg_eval_inputs as SI  # noqa: E402

from egtr_amd import targets as T  # noqa: E402
from egtr_amd.evaluation import SceneGraphRecall, gt_entry  # noqa: E402


def dense_reference_way(triplets, N, R):
    """_get_rel_tensor (visual_genome.py:74-80): zeros, then one indexed assignment."""
    rel = torch.zeros([N, N, R])
    idx = triplets.T
    rel[idx[0, :], idx[1, :], idx[2, :]] = 1.0
    return rel


def random_triplets(g, K, N, R, top_bit=True):
    t = torch.stack([torch.randint(0, N, (K,), generator=g), torch.randint(0, N, (K,), generator=g),
                     torch.randint(0, R, (K,), generator=g)], 1)
    if K >= 4:
        t[1] = t[0]                     # a duplicated triplet
        t[2, :2] = t[0, :2]             # a second predicate on the same pair
        t[2, 2] = (t[0, 2] + 1) % R
        if top_bit:
            t[3, 2] = R - 1             # the highest bit of the word (bit 63 at R = 64)
    return t


def triplets_of_dense(rel, g=None):
    """The triplets of a dense target, shuffled and with a duplicated row when a generator is given."""
    t = rel.nonzero()
    if g is not None and t.shape[0] > 1:
        t = torch.cat([t, t[:1]])[torch.randperm(t.shape[0] + 1, generator=g)]
    return t


@pytest.mark.parametrize("R", [1, 33, 50, 64])
def test_pack_unpack_equals_the_dense_target(R):
    N = 7
    g = torch.Generator().manual_seed(100 + R)
    trips = [random_triplets(g, 9, N, R), torch.zeros(0, 3, dtype=torch.int64), random_triplets(g, 30, N, R)]
    bits = T.pack_relations([{"rel_triplets": t} for t in trips], N, R, "cpu")
    assert bits.dtype == torch.int64 and tuple(bits.shape) == (3, N, N)
    for b, t in enumerate(trips):
        assert torch.equal(T.unpack_relations(bits, b, R), dense_reference_way(t, N, R)), b
    assert int(bits[1].abs().sum()) == 0
    s, o, _ = trips[0][3].tolist()
    word = int(bits[0, s, o])
    assert (word >> (R - 1)) & 1 == 1
    if R == 64:
        assert word < 0                 # bit 63 is the sign bit of the int64 word
    if R < 64:
        assert int((bits >> R).abs().sum()) == 0


def test_relation_triplets_from_a_rel_json_entry():
    rel_list = [[0, 1, 3], [2, 0, 50], [0, 1, 3]]
    t = T.relation_triplets(rel_list)
    assert t.dtype == torch.int64 and t.tolist() == [[0, 1, 2], [2, 0, 49], [0, 1, 2]]
    arr = np.array(rel_list)            # the reference: indices[-1, :] -= 1, then the indexed assignment
    idx = arr.T.copy()
    idx[-1, :] -= 1
    want = torch.zeros(5, 5, 50)
    want[idx[0, :], idx[1, :], idx[2, :]] = 1.0
    assert torch.equal(T.unpack_relations(T.pack_relations([{"rel_triplets": t}], 5, 50, "cpu"), 0, 50), want)
    assert tuple(T.relation_triplets([]).shape) == (0, 3)


@pytest.mark.parametrize("bad", [[7, 0, 0], [0, 7, 0], [0, 0, 5], [-1, 0, 0], [0, -1, 0], [0, 0, -1]])
def test_out_of_range_triplets_raise(bad):
    ok = torch.tensor([[1, 2, 3]])
    with pytest.raises(ValueError):
        T.pack_relations([{"rel_triplets": ok}, {"rel_triplets": torch.tensor([[0, 1, 2], bad])}], 7, 5, "cpu")


def test_more_than_64_predicates_raise():
    with pytest.raises(ValueError):
        T.pack_relations([{"rel_triplets": torch.tensor([[0, 1, 2]])}], 7, 65, "cpu")
    T.pack_relations([{"rel_triplets": torch.tensor([[0, 1, 63]])}], 7, 64, "cpu")


def test_gt_entry_and_recall_from_triplets():
    g = np.load(os.path.join(HERE, "golden", "sgg_eval.npz"))
    _, targets, _ = SI.sgg_eval_inputs(seed=int(g["seed"]))
    gen = torch.Generator().manual_seed(3)
    trip_targets = []
    for t in targets:
        tt = {k: v for k, v in t.items() if k != "rel"}
        tt["rel_triplets"] = triplets_of_dense(t["rel"], gen)
        trip_targets.append(tt)
    assert any(t["rel_triplets"].shape[0] > 1 for t in trip_targets)
    for t, tt in zip(targets, trip_targets):
        a, b = gt_entry(t), gt_entry(tt)
        assert a["gt_relations"].dtype == b["gt_relations"].dtype
        for k in ("gt_relations", "gt_boxes", "gt_classes"):
            assert torch.equal(a[k], b[k]), k
    empty = gt_entry({"class_labels": torch.tensor([1]), "boxes": torch.tensor([[0.5, 0.5, 0.1, 0.1]]),
                      "orig_size": torch.tensor([10, 10]), "rel_triplets": torch.zeros(0, 3, dtype=torch.int64)})
    assert tuple(empty["gt_relations"].shape) == (0, 3)
    for mode in ("m", "s"):
        cands = [{"pred_boxes": torch.from_numpy(g[f"{j}_pred_boxes"]),
                  "pred_classes": torch.from_numpy(g[f"{j}_pred_classes"]),
                  "pred_rel_inds": torch.from_numpy(g[f"{mode}{j}_pred_rel_inds"]),
                  "rel_scores": torch.from_numpy(g[f"{mode}{j}_rel_scores"])} for j in range(len(targets))]
        evs = []
        for tg in (targets, trip_targets):
            ev = SceneGraphRecall(SI.R, multiple_preds=(mode == "m"), keep_per_image=True)
            ev.update(cands, tg)
            evs.append(ev)
        assert torch.equal(evs[0].per_image(), evs[1].per_image())
        assert evs[0].compute() == evs[1].compute()
        assert np.array_equal(evs[0].per_image().numpy(), g[f"{mode}_recall"])


@pytest.mark.parametrize("training", [True, False])
def test_small_model_losses_equal_with_triplet_targets(golden_dir, cpu_kernels, training):
    """Training mode (the sync-light relation route is not taken on CPU tensors: the reference-order route) and evaluation
    mode: every loss term equal exactly; uncertainty within 1e-6 relative (its summation order may differ)."""
    g = Hh.load_golden(golden_dir, "sgg_small.npz")
    cfg_dict, shapes = json.loads(str(g["cfg"])), json.loads(str(g["shapes"]))
    model, cfg, sd = Hh.build_product_model(cfg_dict, shapes, int(g["seed"]))
    model.load_state_dict(sd)
    model.train(training)
    pv, pm = Hh.small_inputs(g)
    dense = W.make_targets(int(g["target_seed"]), 2, cfg.num_queries, cfg.num_labels, cfg.num_rel_labels)
    gen = torch.Generator().manual_seed(9)
    trip = [dict({k: v for k, v in t.items() if k != "rel"}, rel_triplets=triplets_of_dense(t["rel"], gen)) for t in dense]
    out = []
    for targets in (dense, trip):
        torch.manual_seed(0)
        with torch.set_grad_enabled(training):
            out.append(model(pixel_values=pv, pixel_mask=pm, labels=targets, output_attentions=False,
                             output_attention_states=True, output_hidden_states=True))
    a, b = out
    assert set(a.loss_dict) == set(b.loss_dict) and "loss_rel" in a.loss_dict and "uncertainty" in a.loss_dict
    for k in a.loss_dict:
        if k == "uncertainty":
            assert abs(float(a.loss_dict[k]) - float(b.loss_dict[k])) <= 1e-6 * abs(float(a.loss_dict[k]))
        else:
            assert torch.equal(a.loss_dict[k], b.loss_dict[k]), k
    assert torch.equal(a.loss, b.loss)


@pytest.mark.parametrize("neg,nm", [(80, 80), (None, 5)])
def test_device_route_on_cpu_tensors_equal_with_triplet_targets(neg, nm):
    """_loss_relations_device (forced on CPU tensors) and loss_uncertainty called on their own, without forward's cache."""
    from egtr_amd.deformable_detr import DeformableDetrHungarianMatcher
    from egtr_amd.egtr import SceneGraphGenerationLoss
    N, C, R, B = 24, 11, 6, 3
    dense = W.make_targets(21, B, N, C, R, tmin=0, tmax=7)
    dense[1]["rel"].zero_()
    trip = [dict({k: v for k, v in t.items() if k != "rel"}, rel_triplets=triplets_of_dense(t["rel"])) for t in dense]
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(B, N, C, generator=g)
    boxes = torch.rand(B, N, 4, generator=g) * 0.5 + 0.25
    matcher = DeformableDetrHungarianMatcher(class_cost=2, bbox_cost=5, giou_cost=2, smoothing=1e-14)
    indices, costs = matcher({"logits": logits, "pred_boxes": boxes}, dense)
    crit = SceneGraphGenerationLoss(matcher=matcher, num_object_queries=N, num_classes=C, num_rel_labels=R,
                                    eos_coef=0.1, losses=["relations"], smoothing=1e-14, rel_sample_negatives=neg,
                                    rel_sample_nonmatching=nm, model_training=True, focal_alpha=0.25,
                                    rel_sample_negatives_largest=True, rel_sample_nonmatching_largest=True)
    crit.force_device_relations = True
    pr = torch.randn(B, N, N, R, generator=g)
    pc = torch.randn(B, N, N, 1, generator=g)
    a = crit.loss_relations({"pred_rel": pr, "pred_connectivity": pc}, dense, indices, costs, 1.0)
    b = crit.loss_relations({"pred_rel": pr, "pred_connectivity": pc}, trip, indices, costs, 1.0)
    assert torch.equal(a["loss_rel"], b["loss_rel"]) and torch.equal(a["loss_connectivity"], b["loss_connectivity"])
    ua = crit.loss_uncertainty(None, dense, indices, costs, 1.0)["uncertainty"]
    ub = crit.loss_uncertainty(None, trip, indices, costs, 1.0)["uncertainty"]
    assert abs(float(ua) - float(ub)) <= 1e-6 * abs(float(ua))


def test_new_entries_resolve_and_reject_null_arguments():
    from egtr_amd import _lib
    h = _lib.lib()
    assert "egtr_pack_relations_u64" in _lib.SIGNATURES and "egtr_relation_loss_f32" in _lib.SIGNATURES
    assert h.egtr_pack_relations_u64(None, None, None, 2, 3, 7, 5, None) == -1
    words = 1                                                                # EGTR_REL_TARGET_WORDS: the packed target format
    assert h.egtr_relation_loss_f32(None, None, None, None, words, None, None, None, None, 2, 7, 5, 1.0, 80, 80, None, None,
                                    None, None, 0, 0, 0, 0, 0) == -1
    # the packed form is an argument, not an entry of its own: four relation-loss names in the table and in the header
    names = {"egtr_relation_loss_f32", "egtr_relation_loss_workspace_bytes", "egtr_relation_loss_all_f32",
             "egtr_relation_loss_all_workspace_bytes"}
    assert {n for n in _lib.SIGNATURES if n.startswith("egtr_relation_loss")} == names
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "egtr_hip.h")) as f:
        assert set(re.findall(r"\b(egtr_relation_loss\w*)\s*\(", f.read())) == names
    assert h.egtr_abi_version() == 7
