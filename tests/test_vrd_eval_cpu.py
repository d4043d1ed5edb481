"""CPU: the host paths of the phrase- and predicate-detection evaluators (egtr_amd.evaluation.vrd) against the reference's
recorded VRD evaluators (tests/golden/vrd_eval.npz, make_golden_vrd_eval.py): per-image recalls bit-equal, metrics within
the 1e-12 of tests/test_sgg_eval_cpu.py (the same left fold against numpy's pairwise mean); the hand-made images of
vrd_eval_inputs.py; evaluate() with the new flags off; argument errors."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import sgg_eval_inputs as SI  # noqa: E402
import vrd_eval_inputs as VI  # noqa: E402

from egtr_amd.evaluation import (PhraseDetectionRecall, PredicateDetectionRecall, SceneGraphRecall, evaluate,  # noqa: E402
                                 gt_entry, phrase_first_ranks_host, preddet_ranks_host, score_keys_host)
from egtr_amd.kernels.vrd import NO_RANK  # noqa: E402

KS = (1, 20, 50, 100)
CLASSES = {"phrdet": PhraseDetectionRecall, "preddet": PredicateDetectionRecall}


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "vrd_eval.npz"))


@pytest.fixture(scope="module")
def inputs(g):
    targets, phr, prd = VI.vrd_eval_inputs(int(g["seed"]))
    to = lambda entries: [{k: torch.from_numpy(v) for k, v in e.items()} for e in entries]  # noqa: E731
    return targets, {"phrdet": to(phr), "preddet": to(prd)}


def run(mode, cands, targets, groups=((0, 8), (8, 12)), **kw):
    ev = CLASSES[mode](VI.R, ks=KS, **kw)
    for lo, hi in groups:        # images of one candidate count per update
        ev.update(cands[lo:hi], targets[lo:hi])
    return ev


def test_fixture_holds_the_module_inputs(g, inputs):
    targets, cands = inputs
    assert tuple(g["ks"]) == KS
    for j, t in enumerate(targets):
        e = gt_entry(t)
        for k, v in e.items():
            assert np.array_equal(v.numpy(), g[f"{j}_{k}"])
        for pfx, mode in (("phr", "phrdet"), ("prd", "preddet")):
            for k, v in cands[mode][j].items():
                assert np.array_equal(v.numpy(), g[f"{pfx}{j}_{k}"])
    assert any(e["gt_relations"].shape[0] == 9 for e in map(gt_entry, targets))


@pytest.mark.parametrize("mode", ["phrdet", "preddet"])
def test_host_path_matches_reference(g, inputs, mode):
    targets, cands = inputs
    ev = run(mode, cands[mode], targets, keep_per_image=True)
    assert np.array_equal(ev.per_image().numpy(), g[f"{mode}_recall"])          # bit-equal per-image recalls
    got = ev.compute()
    for j, k in enumerate(KS):
        assert abs(got[f"R@{k}"] - g[f"{mode}_stats"][j]) <= 1e-12
    for j, k in enumerate(KS[1:]):
        assert abs(got[f"mR@{k}"] - g[f"{mode}_mr"][j]) <= 1e-12
    assert set(got) == {f"{m}@{k}" for m in ("R", "mR") for k in KS}
    per, ps = ev.per_predicate(), g[f"{mode}_pred_stats"]
    for p in range(VI.R):
        for j, k in enumerate(KS):
            if math.isnan(ps[p, j]):
                assert math.isnan(per[p][f"R@{k}"])
            else:
                assert abs(per[p][f"R@{k}"] - ps[p, j]) <= 1e-12
    nk, want_pp = len(KS), g[f"{mode}_pred_recall"]      # per-image per-predicate recalls, bit for bit
    for j, (c, t) in enumerate(zip(cands[mode], targets)):
        e = CLASSES[mode](VI.R, ks=KS)
        e.update([c], [t])
        for p in range(VI.R):
            if e.acc[e._fbase + p] == 0:
                assert np.isnan(want_pp[p, j]).all()
            else:
                assert np.array_equal(e.acc[e._pbase + p * nk:e._pbase + (p + 1) * nk].numpy(), want_pp[p, j])


def test_fixture_is_nontrivial(g):
    for mode in ("phrdet", "preddet"):
        rec = g[f"{mode}_recall"]
        assert ((rec[:, 1] > 0) & (rec[:, 1] < rec[:, 2]) & (rec[:, 2] < rec[:, 3])).sum() >= 3
        assert np.isnan(g[f"{mode}_pred_stats"][-1]).all()                       # a predicate that never occurs
    assert (g["preddet_recall"][VI.NO_CAND] == 0).all()                          # the image without candidates counts
    # per-predicate ranks differ from the ranks in the whole list somewhere (the mean recall is not a regrouping)
    assert not np.allclose(g["preddet_mr"], g["phrdet_mr"])


def test_phrdet_first_ranks_are_the_references_pred_to_gt(g, inputs):
    targets, cands = inputs
    above = 0
    for j, (c, t) in enumerate(zip(cands["phrdet"], targets)):
        e = gt_entry(t)
        args = (c["pred_rel_inds"], c["pred_boxes"], c["pred_classes"], e["gt_relations"], e["gt_boxes"], e["gt_classes"])
        fr = phrase_first_ranks_host(*args)
        K = c["pred_rel_inds"].shape[0]
        want = torch.full_like(fr, K)
        for cand, gt in g[f"phr{j}_pred_to_gt"].tolist():
            want[gt] = min(int(want[gt]), cand)
        assert torch.equal(fr, want)
        from egtr_amd.evaluation import first_ranks_host
        sg = first_ranks_host(*args)
        assert (fr <= sg).all()              # a union test passes wherever both part tests pass ... on this fixture
        above += int((fr < sg).sum())
    assert above > 0                         # phrdet matches where sgdet does not


def test_phrdet_hand_image():
    cand, target, want, K = VI.phrdet_hand_image()
    e = gt_entry(target)
    fr = phrase_first_ranks_host(cand["pred_rel_inds"], cand["pred_boxes"], cand["pred_classes"], e["gt_relations"],
                                 e["gt_boxes"], e["gt_classes"])
    assert fr.tolist() == want
    ev = PhraseDetectionRecall(4, ks=(1, 2, 3))
    ev.update([cand], [target])
    assert ev.compute()["R@1"] == 1 / 3 and ev.compute()["R@3"] == 2 / 3
    sg = SceneGraphRecall(4, ks=(1, 2, 3), multiple_preds=True)
    sg.update([cand], [target])
    assert sg.compute()["R@3"] == 1 / 3      # the subject of triplet 0 overlaps its GT by 0.25 only


def test_preddet_hand_image_pins_the_tie_rule():
    cand, target, rows, fr, fr_pred = VI.preddet_hand_image()
    e = gt_entry(target)
    got = preddet_ranks_host(cand["pred_rel_inds"], cand["rel_scores"], e["gt_relations"], 4)
    none = lambda xs: [NO_RANK if x is None else x for x in xs]  # noqa: E731
    assert got[0].tolist() == rows and got[1].tolist() == none(fr) and got[2].tolist() == none(fr_pred)
    ev = PredicateDetectionRecall(4, ks=(1, 4, 7, 9))
    ev.update([cand], [target])
    assert ev.compute() == {"R@1": 0.25, "R@4": 0.25, "R@7": 0.5, "R@9": 0.75,
                            "mR@1": 0.25, "mR@4": 0.375, "mR@7": 0.5, "mR@9": 0.5}
    per = ev.per_predicate()                 # p0: ranks 3 and 4 of two triplets; p1: never; p2: rank 0; p3: no GT
    assert per[0] == {"R@1": 0.0, "R@4": 0.5, "R@7": 1.0, "R@9": 1.0} and per[1]["R@9"] == 0.0
    assert per[2]["R@1"] == 1.0 and math.isnan(per[3]["R@1"])


def test_score_keys_order():
    x = torch.tensor([float("nan"), float("-inf"), -1.0, -0.0, 0.0, 1e-30, 0.5, float("inf")])
    k = score_keys_host(x)
    assert k[0] == 0 and k[3] == k[4] and (k[1:4].diff() > 0).all() and (k[4:].diff() > 0).all()


@pytest.mark.parametrize("mode", ["phrdet", "preddet"])
def test_merge_and_batch_size(inputs, mode):
    targets, cands = inputs
    whole = run(mode, cands[mode], targets)
    a = run(mode, cands[mode], targets, groups=((0, 5),))
    a.merge(run(mode, cands[mode], targets, groups=((5, 8), (8, 12))))
    assert torch.allclose(a.acc, whole.acc, rtol=0, atol=1e-12)
    one = run(mode, cands[mode], targets, groups=tuple((i, i + 1) for i in range(12)))
    assert torch.equal(one.acc, whole.acc)
    with pytest.raises(ValueError):
        whole.merge(SceneGraphRecall(VI.R, ks=KS, multiple_preds=True))


@pytest.mark.parametrize("mode", ["phrdet", "preddet"])
def test_zero_gt_image_is_skipped(inputs, mode):
    targets, cands = inputs
    empty = dict(targets[8], rel=torch.zeros_like(targets[8]["rel"]))
    ev = run(mode, cands[mode], targets, groups=((8, 10),), keep_per_image=True)
    ev2 = CLASSES[mode](VI.R, ks=KS, keep_per_image=True)
    ev2.update([cands[mode][8], cands[mode][8], cands[mode][9]], [targets[8], empty, targets[9]])
    assert ev2.skipped == 1 and ev2.n_images == 2 and ev.skipped == 0
    assert torch.equal(ev2.acc[:4], ev.acc[:4]) and torch.equal(ev2.per_image(), ev.per_image())


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def test_evaluate_is_unchanged_with_the_flags_off():
    g = np.load(os.path.join(HERE, "golden", "sgg_eval.npz"))
    outputs, targets, meta = SI.sgg_eval_inputs(seed=int(g["seed"]))
    batches = [{"pixel_values": torch.zeros(len(targets), 3, 8, 8), "pixel_mask": torch.ones(len(targets), 8, 8),
                "labels": targets}]
    args = (_Stub(), batches, meta["num_labels"], meta["num_rel_labels"])
    kw = dict(single=True, multiple=True, graphed=False, forward=lambda pv, pm: outputs)
    base = evaluate(*args, **kw)
    assert set(base) == {f"{p}{m}@{k}" for p in ("", "(single)") for m in ("R", "mR") for k in (20, 50, 100)}
    for j, k in enumerate((20, 50, 100)):      # the values the reference recorded for these inputs
        assert abs(base[f"R@{k}"] - g["m_stats"][j]) <= 1e-12 and abs(base[f"mR@{k}"] - g["m_mr"][j]) <= 1e-12
        assert abs(base[f"(single)R@{k}"] - g["s_stats"][j]) <= 1e-12
        assert abs(base[f"(single)mR@{k}"] - g["s_mr"][j]) <= 1e-12
    assert evaluate(*args, phrdet=False, preddet=False, **kw) == base
    more = evaluate(*args, phrdet=True, **kw)
    assert {k: v for k, v in more.items() if not k.startswith("phrdet_")} == base
    assert set(more) - set(base) == {f"phrdet_{m}@{k}" for m in ("R", "mR") for k in (20, 50, 100)}
    assert all(more[f"phrdet_R@{k}"] >= base[f"R@{k}"] for k in (20, 50, 100))


def test_bad_arguments(inputs):
    targets, cands = inputs
    with pytest.raises(ValueError):
        PredicateDetectionRecall(VI.R, train_counts=torch.zeros(3, 3, VI.R))
    with pytest.raises(ValueError):
        PhraseDetectionRecall(0)
    with pytest.raises(ValueError):
        PredicateDetectionRecall(VI.R, ks=(50, 20))
    phr, prd = cands["phrdet"][0], cands["preddet"][0]
    with pytest.raises(ValueError):          # phrdet takes [K, 3]
        PhraseDetectionRecall(VI.R).update([dict(phr, pred_rel_inds=phr["pred_rel_inds"][:, :2])], targets[:1])
    with pytest.raises(ValueError):          # preddet takes [K, 2]
        PredicateDetectionRecall(VI.R).update([dict(prd, pred_rel_inds=phr["pred_rel_inds"])], targets[:1])
    with pytest.raises(ValueError):
        PredicateDetectionRecall(VI.R).update([dict(prd, rel_scores=prd["rel_scores"][:, :3])], targets[:1])
    big = torch.zeros(1025, 3, dtype=torch.long)
    with pytest.raises(ValueError):
        PhraseDetectionRecall(VI.R).update([dict(phr, pred_rel_inds=big)], targets[:1])
    with pytest.raises(ValueError):
        PredicateDetectionRecall(VI.R).update(
            [dict(pred_rel_inds=big[:, :2], rel_scores=torch.zeros(1025, VI.R))], targets[:1])
    with pytest.raises(KeyError):
        PredicateDetectionRecall(VI.R).update([{"pred_rel_inds": prd["pred_rel_inds"]}], targets[:1])
    with pytest.raises(ValueError):
        PredicateDetectionRecall(VI.R).update([prd, prd], targets[:1])
    with pytest.raises(RuntimeError):
        PredicateDetectionRecall(VI.R).zero_shot()
