"""Golden vectors of the Open Images relation metrics, produced by RUNNING THE REFERENCE:

  * train_egtr.evaluate_batch (train_egtr.py:43-175) is imported from the reference tree with the inert mocks of
    make_golden_post.py for its import-time dependencies -- except lib.evaluation.oi_eval, lib.evaluation.ap_eval_rel and
    lib.evaluation.sg_eval, which are the REAL modules here (pycocotools, which eval_rel_results never touches, is mocked
    inertly); sg_eval's native dependency lib.fpn.box_intersections_cpu.bbox is the reference's Cython source compiled by
    oracle/Makefile (oracle.ref_bbox.load()).
  * evaluate_batch drives a real OIEvaluator; eval_rel_results(ev.all_result, predicates) gives the metrics.  Internals
    are recorded by wrapping module attributes: _compute_pred_matches (per-image pred_to_gt), prepare_mAP_dets (the
    per-image detections it receives, the per-class records and npos) and ap_eval (rec, prec, ap per class and mode).

    make -C oracle ref && python tests/golden/make_golden_oi_eval.py      -> tests/golden/oi_eval.npz"""
import contextlib
import hashlib
import io
import os
import sys
from functools import reduce
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden_post  # noqa: E402
import oi_eval_inputs as OI  # noqa: E402

KS = (1, 5, 10, 20, 50, 100)


def import_reference():
    from oracle import ref_bbox
    bbox = ref_bbox.load()
    assert bbox is not None, "run `make -C oracle ref` first"
    import _ref_import
    _ref_import.load_reference()
    sys.modules["lib.fpn.box_intersections_cpu.bbox"] = bbox
    for name in ("pycocotools", "pycocotools.coco", "pycocotools.cocoeval"):
        sys.modules.setdefault(name, mock.MagicMock(name=name))
    import lib.evaluation.oi_eval as oi_eval   # the real modules (imported before the mocks are installed)
    te = make_golden_post.import_train_egtr()
    assert sys.modules["lib.evaluation.oi_eval"] is oi_eval
    return te, oi_eval


def main():
    te, oi_eval = import_reference()
    outputs, targets, meta = OI.oi_eval_inputs(seed=83)
    R = meta["num_rel_labels"]
    ev = oi_eval.OIEvaluator(list(range(R)), list(range(meta["num_labels"])))
    te.evaluate_batch(outputs, targets, None, [], None, [], ev, meta["num_labels"], max_topk=100)
    assert len(ev.all_result) == len(targets)
    res = {}
    for j, r in enumerate(ev.all_result):
        n = len(r["pred_boxes"])
        OI.check_ties(r["pred_scores"], r["pred_cls_scores"], np.stack([np.arange(n * n) // n, np.arange(n * n) % n], 1))
        for k in ("pred_boxes", "pred_class", "pred_cls_scores", "gt_boxes", "gt_class", "gt_prd_labels"):
            res[f"img{j}_{k}"] = np.asarray(r[k])
        # pred_scores (123 KB of random floats per image) is rebuilt from the seeded inputs by the tests; its digest
        # pins the rebuild to what the reference evaluated
        res[f"img{j}_pred_scores_sha256"] = np.asarray(hashlib.sha256(
            np.ascontiguousarray(r["pred_scores"], np.float32).tobytes()).hexdigest())

    matches, dets_in, prep, aps = [], [], {}, {}
    real_match, real_prep, real_ap = oi_eval._compute_pred_matches, oi_eval.prepare_mAP_dets, oi_eval.ap_eval

    def rec_match(*a, **k):
        out = real_match(*a, **k)
        matches.append((len(a[0]), out))
        return out

    def rec_prep(topk_dets, cls_num):
        dets_in.extend(topk_dets)
        out = real_prep(topk_dets, cls_num)
        prep["out"] = out
        return out

    def rec_ap(image_ids, dets, gts, npos, rel_or_phr=True, ovthresh=0.5):
        rec, prec, ap = real_ap(image_ids, dets, gts, npos, rel_or_phr, ovthresh)
        aps[(len(aps) % R, "rel" if rel_or_phr else "phr")] = (np.asarray(rec), np.asarray(prec), float(ap))
        return rec, prec, ap

    oi_eval._compute_pred_matches, oi_eval.prepare_mAP_dets, oi_eval.ap_eval = rec_match, rec_prep, rec_ap
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        metrics = oi_eval.eval_rel_results(ev.all_result, list(range(R)))
    oi_eval._compute_pred_matches, oi_eval.prepare_mAP_dets, oi_eval.ap_eval = real_match, real_prep, real_ap
    assert len(matches) == len(targets) and len(aps) == 2 * R

    per_img = np.zeros((len(targets), len(KS)))
    for j, ((n_gt, p2g), d) in enumerate(zip(matches, dets_in)):
        K = len(d["det_scores_top"])
        res[f"det{j}_labels"] = np.stack([d["det_labels_s_top"], d["det_labels_p_top"], d["det_labels_o_top"]], 1)
        res[f"det{j}_boxes"] = np.hstack([d["det_boxes_s_top"], d["det_boxes_o_top"]])
        res[f"det{j}_scores"] = np.asarray(d["det_scores_top"], np.float32)
        m = np.zeros((K, n_gt), bool)
        for i, gl in enumerate(p2g):
            m[i, gl] = True
        res[f"det{j}_pred_to_gt"] = m
        for q, k in enumerate(KS):
            hit = reduce(np.union1d, p2g[:k]) if len(p2g) else []
            per_img[j, q] = float(len(hit)) / float(n_gt + 1e-12)
    res["per_image_recall"] = per_img
    cls_image_ids, cls_dets, _, npos = prep["out"]
    res["npos"] = np.asarray(npos)
    for c in range(R):
        res[f"cls{c}_image_ids"] = np.asarray(cls_image_ids[c], np.int64)
        res[f"cls{c}_confidence"] = np.asarray(cls_dets[c]["confidence"])
        conf = res[f"cls{c}_confidence"]
        assert len(np.unique(conf)) == len(conf), f"tie between confidences of class {c}"
        for mode in ("rel", "phr"):
            rec, prec, ap = aps[(c, mode)]
            res[f"cls{c}_{mode}_rec"] = rec
            res[f"cls{c}_{mode}_prec"] = prec
            res[f"cls{c}_{mode}_ap"] = np.float64(ap)
    for k, v in metrics.items():
        res[f"metric_{k}"] = np.float64(v)
    res["metric_rel_mAP"] = np.float64(sum(aps[(c, "rel")][2] for c in range(R)) / R)
    res["metric_phr_mAP"] = np.float64(sum(aps[(c, "phr")][2] for c in range(R)) / R)
    np.savez_compressed(os.path.join(HERE, "oi_eval.npz"), seed=83, **res)
    print({k: float(v) for k, v in res.items() if k.startswith("metric_")})
    print("per-class npos", res["npos"])
    print("per-image R@k mean", per_img.mean(0))


if __name__ == "__main__":
    main()
