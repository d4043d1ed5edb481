"""Golden vectors of the scene-graph evaluator (Recall@K / mean Recall@K), produced by RUNNING THE REFERENCE:

  * train_egtr.evaluate_batch (train_egtr.py:43-139) is imported from the reference tree with the inert mocks of
    make_golden_post.py for its import-time dependencies -- except lib.evaluation.sg_eval, which is the REAL module here;
    its native dependency lib.fpn.box_intersections_cpu.bbox is the reference's Cython source compiled by oracle/Makefile
    (oracle.ref_bbox.load()).
  * evaluate_batch drives the real BasicSceneGraphEvaluator in both modes (single- and multiple-predicate) plus one
    per-predicate evaluator per predicate (evaluate_egtr.py:53-63); the final numbers come from print_stats and
    calculate_mR_from_evaluator_list.

    make -C oracle ref && python tests/golden/make_golden_sgg_eval.py      -> tests/golden/sgg_eval.npz

Stored: each evaluator's per-image result lists, the final R@k / mR@k dicts, the pred_entry / gt_entry the reference
built for each image; for the regular inputs and for the chain variant (sgg_eval_inputs.py)."""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden_post  # noqa: E402
import sgg_eval_inputs as SI  # noqa: E402

KS = (20, 50, 100)


def import_reference():
    from oracle import ref_bbox
    bbox = ref_bbox.load()
    assert bbox is not None, "run `make -C oracle ref` first"
    import _ref_import
    _ref_import.load_reference()
    sys.modules["lib.fpn.box_intersections_cpu.bbox"] = bbox
    import lib.evaluation.sg_eval as sg_eval   # the real module (imported before the mocks are installed)
    te = make_golden_post.import_train_egtr()
    assert sys.modules["lib.evaluation.sg_eval"] is sg_eval
    return te, sg_eval


def run(te, sg_eval, prefix, outputs, targets, meta, res):
    R = meta["num_rel_labels"]
    evs = {"m": sg_eval.BasicSceneGraphEvaluator.all_modes(multiple_preds=True),
           "s": sg_eval.BasicSceneGraphEvaluator.all_modes(multiple_preds=False)}
    lists = {m: [(p, f"p{p}", sg_eval.BasicSceneGraphEvaluator.all_modes(multiple_preds=(m == "m"))) for p in range(R)]
             for m in evs}
    entries = {m: [] for m in evs}
    for m, ev in evs.items():
        inner = ev["sgdet"].evaluate_scene_graph_entry

        def rec(gt_entry, pred_entry, _inner=inner, _m=m, **kw):
            entries[_m].append((gt_entry, pred_entry))
            return _inner(gt_entry, pred_entry, **kw)
        ev["sgdet"].evaluate_scene_graph_entry = rec
    te.evaluate_batch(outputs, targets, evs["m"], lists["m"], evs["s"], lists["s"], None, meta["num_labels"],
                      max_topk=100)
    B = len(targets)
    with contextlib.redirect_stdout(io.StringIO()):
        for m in evs:
            stats = evs[m]["sgdet"].print_stats()
            mr = sg_eval.calculate_mR_from_evaluator_list(lists[m], "sgdet", multiple_preds=(m == "m"))
            res[f"{prefix}{m}_stats"] = np.array([stats[f"R@{k}"] for k in KS])
            res[f"{prefix}{m}_mr"] = np.array([mr[f"mR@{k}"] for k in KS])
            res[f"{prefix}{m}_pred_stats"] = np.array([[ev["sgdet"].print_stats()[f"R@{k}"] for k in KS]
                                                       for _, _, ev in lists[m]])
            res[f"{prefix}{m}_recall"] = np.array([evs[m]["sgdet"].result_dict["sgdet_recall"][k] for k in KS]).T
            # per-predicate per-image recalls: [R, B, nk], NaN where the image has no GT triplet of p
            per = np.full((R, B, len(KS)), np.nan)
            for p, _, ev in lists[m]:
                rd = ev["sgdet"].result_dict["sgdet_recall"]
                imgs = [j for j, (gt, _) in enumerate(entries[m]) if (gt["gt_relations"][:, 2] == p).any()]
                assert len(imgs) == len(rd[20])
                for i, j in enumerate(imgs):
                    per[p, j] = [rd[k][i] for k in KS]
            res[f"{prefix}{m}_pred_recall"] = per
            for j, (gt, pred) in enumerate(entries[m]):
                res[f"{prefix}{m}{j}_pred_rel_inds"] = np.asarray(pred["pred_rel_inds"])
                res[f"{prefix}{m}{j}_rel_scores"] = np.asarray(pred["rel_scores"], dtype=np.float32)
                if m == "m":
                    res[f"{prefix}{j}_pred_boxes"] = np.asarray(pred["pred_boxes"])
                    res[f"{prefix}{j}_pred_classes"] = np.asarray(pred["pred_classes"])
                    for k, v in gt.items():
                        res[f"{prefix}{j}_{k}"] = np.asarray(v)


def main():
    te, sg_eval = import_reference()
    res = {}
    for prefix, chain in (("", False), ("chain_", True)):
        outputs, targets, meta = SI.sgg_eval_inputs(seed=71, chain=chain)
        run(te, sg_eval, prefix, outputs, targets, meta, res)
    np.savez_compressed(os.path.join(HERE, "sgg_eval.npz"), seed=71, **res)
    for pfx in ("", "chain_"):
        print(pfx, "multiple R@k", res[f"{pfx}m_stats"], "mR@k", res[f"{pfx}m_mr"])
        print(pfx, "single   R@k", res[f"{pfx}s_stats"], "mR@k", res[f"{pfx}s_mr"])
    print("per-image single recalls", res["s_recall"])


if __name__ == "__main__":
    main()
