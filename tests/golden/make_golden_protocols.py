"""Golden vectors of the PredCls / SGCls protocols, produced by RUNNING THE REFERENCE'S EVALUATOR:

  * lib.evaluation.sg_eval is the real module of the reference tree (its native dependency
    lib.fpn.box_intersections_cpu.bbox is the reference's Cython source compiled by oracle/Makefile), and
    lib.pytorch_misc.argsort_desc is the reference's ranking;
  * per image the UNPADDED candidate list is built here with numpy, restating train_egtr.py:57-69 / 86-94 / 122-128 on
    the sub-tensor of the matched queries (protocols_eval_inputs.py gives GT object -> query explicitly): object scores
    1 and GT classes for "predcls", the matched query's softmax score and class for "sgcls"; the zero-score self pairs
    the reference keeps at the end of its ranking are dropped, as the package's definition leaves them out;
  * BasicSceneGraphEvaluator(mode="predcls" | "sgcls", multiple_preds=True | False) scores the lists, one more evaluator
    per predicate is fed the GT list filtered by that predicate (train_egtr.py:111-119), and the final numbers come from
    print_stats and calculate_mR_from_evaluator_list.

    make -C oracle ref && python tests/golden/make_golden_protocols.py      -> tests/golden/protocols_eval.npz

Stored (data only): per image, protocol and mode the list (pred_rel_inds, rel_scores, triplet_scores) with the object
classes and scores it was built from, every evaluator's per-image recalls, the final R@k / mR@k.  numpy's argsort is
unstable, so the generator asserts what makes the lists well defined: inside every image's domain all scores are > 0 and
pairwise distinct; and every image has a GT relation (the reference asserts it)."""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import protocols_eval_inputs as PI  # noqa: E402

KS = (20, 50, 100)
PROTOCOLS = ("predcls", "sgcls")
MODES = (("m", True), ("s", False))
SEED = 97
MAX_TOPK = 100


def import_reference():
    from oracle import ref_bbox
    bbox = ref_bbox.load()
    assert bbox is not None, "run `make -C oracle ref` first"
    import _ref_import
    _ref_import.load_reference()
    sys.modules["lib.fpn.box_intersections_cpu.bbox"] = bbox
    import lib.evaluation.sg_eval as sg_eval
    from lib.pytorch_misc import argsort_desc
    return sg_eval, argsort_desc


def candidate_lists(argsort_desc, outputs, j, query_of, gt_classes, protocol):
    """The two unpadded lists (multiple, single) of image j in GT-object numbering."""
    q = np.asarray(query_of, np.int64)
    G = q.shape[0]
    rel = np.clip(outputs["pred_rel"][j].numpy(), 0.0, 1.0)
    conn = np.clip(outputs["pred_connectivity"][j].numpy(), 0.0, 1.0)
    pred_rel = (rel * conn)[q][:, q]                                       # [G, G, R] float32
    if protocol == "predcls":
        obj_scores, classes = np.ones(G, np.float32), np.asarray(gt_classes, np.int64)
    else:
        sc, cl = torch.max(outputs["logits"][j].softmax(-1)[:, :PI.NUM_LABELS], -1)
        obj_scores, classes = sc.numpy()[q], cl.numpy()[q]
    sub_ob = np.outer(obj_scores, obj_scores).astype(np.float32)
    sub_ob[np.arange(G), np.arange(G)] = 0.0
    off = ~np.eye(G, dtype=bool)
    out = {}
    trip = pred_rel * sub_ob[..., None]
    dom = trip[off].ravel()
    assert (dom > 0).all() and np.unique(dom).size == dom.size, "tied or zero triplet scores"
    inds = argsort_desc(trip)
    inds = inds[inds[:, 0] != inds[:, 1]][:MAX_TOPK]
    out["m"] = dict(pred_rel_inds=inds, rel_scores=pred_rel[inds[:, 0], inds[:, 1], inds[:, 2]],
                    triplet_scores=trip[inds[:, 0], inds[:, 1], inds[:, 2]])
    pair = pred_rel.max(-1) * sub_ob
    dom = pair[off].ravel()
    assert (dom > 0).all() and np.unique(dom).size == dom.size, "tied or zero pair scores"
    inds = argsort_desc(pair)
    inds = inds[inds[:, 0] != inds[:, 1]][:MAX_TOPK]
    out["s"] = dict(pred_rel_inds=inds, rel_scores=pred_rel[inds[:, 0], inds[:, 1]],
                    triplet_scores=pair[inds[:, 0], inds[:, 1]])
    for e in out.values():
        e.update(pred_classes=classes, obj_scores=obj_scores)
    return out


def main():
    sg_eval, argsort_desc = import_reference()
    from egtr_amd.evaluation import gt_entry
    outputs, targets, query_of = PI.protocols_eval_inputs(SEED)
    B, R = len(targets), PI.R
    res = {}
    for proto in PROTOCOLS:
        evs = {m: sg_eval.BasicSceneGraphEvaluator(mode=proto, multiple_preds=mp) for m, mp in MODES}
        lists = {m: [(p, f"p{p}", {proto: sg_eval.BasicSceneGraphEvaluator(mode=proto, multiple_preds=mp)})
                     for p in range(R)] for m, mp in MODES}
        per = {m: np.full((R, B, len(KS)), np.nan) for m, _ in MODES}
        for j, t in enumerate(targets):
            gt = {k: v.numpy() for k, v in gt_entry(t).items()}
            assert gt["gt_relations"].shape[0] > 0
            cands = candidate_lists(argsort_desc, outputs, j, query_of[j], gt["gt_classes"], proto)
            for m, _ in MODES:
                entry = dict(cands[m], pred_boxes=gt["gt_boxes"])
                evs[m].evaluate_scene_graph_entry(gt, entry)
                for p, _, ev_p in lists[m]:
                    mask = gt["gt_relations"][:, 2] == p
                    if not mask.any():
                        continue
                    ev_p[proto].evaluate_scene_graph_entry(dict(gt, gt_relations=gt["gt_relations"][mask]), entry)
                    per[m][p, j] = [ev_p[proto].result_dict[proto + "_recall"][k][-1] for k in KS]
                for k, v in cands[m].items():
                    res[f"{proto}_{m}{j}_{k}"] = np.asarray(v)
            if proto == PROTOCOLS[0]:
                for k, v in gt.items():
                    res[f"{j}_{k}"] = v
                res[f"{j}_query_of"] = np.asarray(query_of[j])
        with contextlib.redirect_stdout(io.StringIO()):
            for m, mp in MODES:
                stats = evs[m].print_stats()
                mr = sg_eval.calculate_mR_from_evaluator_list(lists[m], proto, multiple_preds=mp)
                res[f"{proto}_{m}_stats"] = np.array([stats[f"R@{k}"] for k in KS])
                res[f"{proto}_{m}_mr"] = np.array([mr[f"mR@{k}"] for k in KS])
                res[f"{proto}_{m}_pred_stats"] = np.array([[e[proto].print_stats()[f"R@{k}"] for k in KS]
                                                           for _, _, e in lists[m]])
                res[f"{proto}_{m}_recall"] = np.array([evs[m].result_dict[proto + "_recall"][k] for k in KS]).T
                res[f"{proto}_{m}_pred_recall"] = per[m]
    path = os.path.join(HERE, "protocols_eval.npz")
    np.savez_compressed(path, seed=SEED, ks=np.array(KS), **res)
    for proto in PROTOCOLS:
        for m, _ in MODES:
            print(proto, m, "R@k", res[f"{proto}_{m}_stats"], "mR@k", res[f"{proto}_{m}_mr"])
            print(proto, m, "per-image", res[f"{proto}_{m}_recall"].tolist())
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
