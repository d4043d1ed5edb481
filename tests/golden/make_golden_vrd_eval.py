"""Golden vectors of the phrase- and predicate-detection evaluators, produced by RUNNING THE REFERENCE:

  * lib.evaluation.sg_eval is the real module of the reference tree; its native dependency
    lib.fpn.box_intersections_cpu.bbox is the reference's Cython source compiled by oracle/Makefile
    (oracle.ref_bbox.load()).
  * BasicSceneGraphEvaluator.vrd_modes() gives the "phrdet" and "preddet" evaluators; one more vrd_modes() per predicate
    is fed the GT list filtered by that predicate, the way the reference's drivers feed their per-predicate evaluators
    (train_egtr.py:111-119); the final numbers come from print_stats and calculate_mR_from_evaluator_list.  The
    evaluators' result lists get the extra key 1 beside 20 / 50 / 100 (data of the instance: the recall at k = 1).

    make -C oracle ref && python tests/golden/make_golden_vrd_eval.py      -> tests/golden/vrd_eval.npz

Stored (data only): the inputs (vrd_eval_inputs.py) and the gt_entry of each image, every evaluator's per-image recalls,
the final R@k / mR@k, and for phrdet the pred_to_gt lists as (candidate, GT triplet) rows.  The generator asserts what the
fixture relies on: no two preddet list entries of an image carry the same score, and both protocols have a first match
at candidate 64."""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import vrd_eval_inputs as VI  # noqa: E402

KS = (1, 20, 50, 100)
MODES = ("phrdet", "preddet")
SEED = 83


def import_reference():
    from oracle import ref_bbox
    bbox = ref_bbox.load()
    assert bbox is not None, "run `make -C oracle ref` first"
    import _ref_import
    _ref_import.load_reference()
    sys.modules["lib.fpn.box_intersections_cpu.bbox"] = bbox
    import lib.evaluation.sg_eval as sg_eval
    return sg_eval


def new_evaluators(sg_eval):
    evs = sg_eval.BasicSceneGraphEvaluator.vrd_modes()
    for m, ev in evs.items():
        assert ev.multiple_preds
        ev.result_dict[m + "_recall"] = {k: [] for k in KS}
    return evs


def assert_no_tied_entries(gt_rels, prd):
    pairs, scores = prd["pred_rel_inds"], prd["rel_scores"]
    if pairs.shape[0] == 0:
        return
    prc = (pairs[:, None, :] == gt_rels[None, :, :2]).all(2)
    entries = scores[prc.argmax(0)].ravel()
    assert np.unique(entries).size == entries.size, "tied preddet scores: numpy's argsort order is not defined"


def main():
    sg_eval = import_reference()
    from egtr_amd.evaluation import gt_entry
    targets, phr, prd = VI.vrd_eval_inputs(SEED)
    B, R = len(targets), VI.R
    evs = new_evaluators(sg_eval)
    lists = [(p, f"p{p}", new_evaluators(sg_eval)) for p in range(R)]
    per = {m: np.full((R, B, len(KS)), np.nan) for m in MODES}
    res = {}
    first64 = {m: False for m in MODES}
    for j, t in enumerate(targets):
        gt = {k: v.numpy() for k, v in gt_entry(t).items()}
        entry = {"phrdet": phr[j], "preddet": prd[j]}
        assert_no_tied_entries(gt["gt_relations"], prd[j])
        pred_to_gt, _, _ = evs["phrdet"].evaluate_scene_graph_entry(gt, phr[j])
        evs["preddet"].evaluate_scene_graph_entry(gt, prd[j])
        rows = np.array([(c, g) for c, gs in enumerate(pred_to_gt) for g in gs], np.int64).reshape(-1, 2)
        res[f"phr{j}_pred_to_gt"] = rows
        if rows.shape[0]:
            firsts = [rows[rows[:, 1] == g, 0].min() for g in np.unique(rows[:, 1])]
            first64["phrdet"] |= 64 in firsts
        if prd[j]["pred_rel_inds"].shape[0]:
            prc = (prd[j]["pred_rel_inds"][:, None, :] == gt["gt_relations"][None, :, :2]).all(2)
            first64["preddet"] |= bool(((prc.argmax(0) == 64) & prc.any(0)).any())
        for p, _, ev_p in lists:
            mask = gt["gt_relations"][:, 2] == p
            if not mask.any():
                continue
            gt_p = dict(gt, gt_relations=gt["gt_relations"][mask])
            for m in MODES:
                ev_p[m].evaluate_scene_graph_entry(gt_p, entry[m])
                per[m][p, j] = [ev_p[m].result_dict[m + "_recall"][k][-1] for k in KS]
        for k, v in gt.items():
            res[f"{j}_{k}"] = v
        for k, v in phr[j].items():
            res[f"phr{j}_{k}"] = v
        for k, v in prd[j].items():
            res[f"prd{j}_{k}"] = v
    assert all(first64.values()), first64
    with contextlib.redirect_stdout(io.StringIO()):
        for m in MODES:
            stats = evs[m].print_stats()
            mr = sg_eval.calculate_mR_from_evaluator_list([(p, n, e) for p, n, e in lists], m, multiple_preds=True)
            res[f"{m}_stats"] = np.array([stats[f"R@{k}"] for k in KS])
            res[f"{m}_mr"] = np.array([mr[f"mR@{k}"] for k in KS[1:]])
            res[f"{m}_pred_stats"] = np.array([[e[m].print_stats()[f"R@{k}"] for k in KS] for _, _, e in lists])
            res[f"{m}_recall"] = np.array([evs[m].result_dict[m + "_recall"][k] for k in KS]).T
            res[f"{m}_pred_recall"] = per[m]
    path = os.path.join(HERE, "vrd_eval.npz")
    np.savez_compressed(path, seed=SEED, ks=np.array(KS), **res)
    for m in MODES:
        print(m, "R@k", res[f"{m}_stats"], "mR@k", res[f"{m}_mr"])
        print(m, "per-image", res[f"{m}_recall"].tolist())
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
