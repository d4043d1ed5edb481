"""Evaluation metrics accumulated where the model outputs live, one module per metric, each with its HIP kernels and a
host implementation of the same semantics (the module docstrings state them):
  * ``sgg``   scene-graph Recall@K / mean Recall@K (``SceneGraphRecall``; csrc/sgg_eval.hip);
  * ``oi``    Open Images relation mAP / recall / score (``OpenImagesRelationMetrics``; csrc/oi_eval.hip);
  * ``coco``  COCO box-detection AP / AR (``CocoDetectionMetrics``; csrc/coco_eval.hip);
  * PredCls / SGCls: ``SceneGraphRecall`` itself, on ``runtime.matched_triplet_candidates`` (csrc/matched_topk.hip);
  * ``vrd``   phrase- and predicate-detection recall (``PhraseDetectionRecall``, ``PredicateDetectionRecall``;
    csrc/vrd_eval.hip);
  * ``_common``  what they share: the GT entry, the first-rank matching, staging, accumulator, checks, record exchange.
``evaluate`` below drives a model over batches and scores whichever of them are enabled.
"""
import types

import torch

from ._common import (_MAX_CAND, _MAX_K, _MAX_REL, _bbox_iou_pyx, _tensor, first_ranks_host, gt_entry, numpy_argmax,  # noqa: F401
                      rescale_bboxes, seen_bits_host)
from .coco import (_COCO_MAX_CLS, _COCO_MAX_DET, _COCO_MAX_GT, _EPS, COCO_AREA_RNGS, COCO_IOU_THRS, COCO_MAX_DETS,  # noqa: F401
                   COCO_REC_THRS, COCO_STATS, CocoDetectionMetrics, _coco_gt, _score_key, _segment_rank,
                   coco_accumulate_host, coco_gt_entry, coco_iou_host, coco_match_host, coco_summarize)
from .oi import (_OI_MAX_GT, _OI_MAX_PAIRS, _OI_MAX_PRDK, _OI_MAX_TOPK, OpenImagesRelationMetrics, _union,  # noqa: F401
                 bbox_iou_f32, oi_ap_host, oi_select_host, oi_tp_host)
from .sgg import SceneGraphRecall, _check_candidate  # noqa: F401
from .vrd import (PhraseDetectionRecall, PredicateDetectionRecall, phrase_first_ranks_host, preddet_ranks_host,  # noqa: F401
                  score_keys_host)


@torch.no_grad()
def evaluate(model, batches, num_labels, num_rel_labels, single=True, multiple=False, max_topk=100, graphed=True,
             forward=None, oi=False, coco=False, feature_extractor=None, train_counts=None, phrdet=False, preddet=False,
             matcher=None, predcls=False, sgcls=False):
    """The Visual Genome path of the reference's ``evaluate`` (evaluate_egtr.py:40-127): run the model over ``batches``
    (the reference's collate_fn format: pixel_values, pixel_mask, labels), build the candidates on the device
    (``runtime.triplet_candidates``) and score them.  Returns the reference's ``metric_dict`` keys: ``R@k`` / ``mR@k``
    of the multiple-predicate evaluator and ``(single)R@k`` / ``(single)mR@k`` of the single-predicate one.  The
    model runs through a ``GraphedForward`` when ``graphed`` (and a GPU is present); one created here is released before
    returning (``forward``: an existing ``GraphedForward`` to reuse instead, left as it is).  ``oi``: also score the
    Open Images branch (``OpenImagesRelationMetrics`` on ``triplet_candidates(mode="oi")``) and add its keys --
    w_rel_mAP, w_phr_mAP, microR@50, score, rel_mAP, phr_mAP, microR@k, and the per-image mean recalls as (oi)R@k.
    ``coco``: also score the boxes (``feature_extractor.post_process`` with the targets' orig_size, default a
    ``DeformableDetrFeatureExtractor``, into ``CocoDetectionMetrics(num_labels)``) and add the reference's "AP50".
    ``train_counts``: a ``RelationStatistics`` / ``fg_matrix`` of the training set (``SceneGraphRecall(train_counts=...)``);
    adds the zero-shot recalls ``zR@k`` (multiple) and ``(single)zR@k``.
    ``phrdet``: also score phrase detection (``PhraseDetectionRecall`` on the "multiple" candidates) and add
    ``phrdet_R@k`` / ``phrdet_mR@k`` (and ``phrdet_zR@k`` with ``train_counts``).  ``preddet``: also score predicate
    detection (``PredicateDetectionRecall`` on ``runtime.matched_pair_candidates``: the GT objects matched to queries by
    ``matcher``, default the model's own Hungarian matcher) and add ``preddet_R@k`` / ``preddet_mR@k``.
    ``predcls`` / ``sgcls``: also score the PredCls / SGCls protocol (``SceneGraphRecall`` on
    ``runtime.matched_triplet_candidates``: GT boxes, the GT objects matched to queries by ``matcher``).  ``multiple`` and
    ``single`` select the evaluators as they do for sgdet -- at least one must be on -- and the keys are ``predcls_R@k`` /
    ``predcls_mR@k`` (``predcls_zR@k`` with ``train_counts``), ``(single)predcls_...`` for the single-predicate
    evaluator, and the same with ``sgcls_``."""
    from ..runtime import GraphedForward, matched_pair_candidates, matched_triplet_candidates, triplet_candidates
    if not (single or multiple or oi or coco or phrdet or preddet):
        raise ValueError("enable at least one of single / multiple / oi / coco / phrdet / preddet")
    protocols = [name for name, on in (("predcls", predcls), ("sgcls", sgcls)) if on]
    if protocols and not (single or multiple):
        raise ValueError("predcls / sgcls need at least one of single / multiple")
    model.eval()
    device = next(model.parameters()).device
    ev_s = SceneGraphRecall(num_rel_labels, multiple_preds=False, train_counts=train_counts) if single else None
    ev_m = SceneGraphRecall(num_rel_labels, multiple_preds=True, train_counts=train_counts) if multiple else None
    ev_oi = OpenImagesRelationMetrics(num_rel_labels) if oi else None
    ev_coco = CocoDetectionMetrics(num_labels) if coco else None
    ev_phr = PhraseDetectionRecall(num_rel_labels, train_counts=train_counts) if phrdet else None
    ev_prd = PredicateDetectionRecall(num_rel_labels) if preddet else None
    # (protocol, candidate mode, key prefix) -> evaluator
    ev_proto = {(name, mode, prefix): SceneGraphRecall(num_rel_labels, multiple_preds=(mode == "multiple"),
                                                       train_counts=train_counts)
                for name in protocols for mode, prefix, on in (("multiple", "", multiple), ("single", "(single)", single))
                if on}
    if (preddet or protocols) and matcher is None:
        matcher = model._matcher()
    if coco and feature_extractor is None:
        from ..feature_extraction import DeformableDetrFeatureExtractor
        feature_extractor = DeformableDetrFeatureExtractor()
    fwd = forward
    own = fwd is None and graphed and device.type == "cuda"
    if own:
        fwd = GraphedForward(model, enabled=True, strict=False)
    try:
        for batch in batches:
            pv = batch["pixel_values"].to(device, non_blocking=True)
            pm = batch["pixel_mask"].to(device, non_blocking=True)
            if fwd is not None:
                outputs = fwd(pv, pm)
            else:
                outputs = model(pixel_values=pv, pixel_mask=pm, output_attentions=False, output_attention_states=True,
                                output_hidden_states=True)
            targets = batch["labels"]
            sizes = torch.stack([torch.as_tensor(t["orig_size"]).cpu() for t in targets])
            if device.type == "cuda":   # a pageable host -> device copy would wait for the stream
                sizes = sizes.pin_memory().to(device, non_blocking=True)
            if ev_m is not None or ev_phr is not None:
                cands_m = triplet_candidates(outputs, num_labels, sizes, max_topk, mode="multiple")
                if ev_m is not None:
                    ev_m.update(cands_m, targets)
                if ev_phr is not None:
                    ev_phr.update(cands_m, targets)
            if ev_prd is not None:
                ev_prd.update(matched_pair_candidates(outputs, targets, matcher, num_labels), targets)
            for (name, mode, _), ev in ev_proto.items():
                ev.update(matched_triplet_candidates(outputs, targets, matcher, num_labels, max_topk, mode=mode,
                                                     protocol=name), targets)
            if ev_s is not None:
                ev_s.update(triplet_candidates(outputs, num_labels, sizes, max_topk, mode="single"), targets)
            if ev_oi is not None:
                ev_oi.update(triplet_candidates(outputs, num_labels, sizes, max_topk, mode="oi"), targets)
            if ev_coco is not None:
                boxes_out = types.SimpleNamespace(logits=outputs["logits"], pred_boxes=outputs["pred_boxes"])
                ev_coco.update(feature_extractor.post_process(boxes_out, sizes), targets)
    finally:
        if own:
            fwd.close()
    metrics = {}
    if ev_m is not None:
        metrics.update(ev_m.compute())
        metrics.update(ev_m.mean_recall())
        if train_counts is not None:
            metrics.update(ev_m.zero_shot())
    if ev_s is not None:
        metrics.update({f"(single){k}": v for k, v in ev_s.compute().items()})
        metrics.update({f"(single){k}": v for k, v in ev_s.mean_recall().items()})
        if train_counts is not None:
            metrics.update({f"(single){k}": v for k, v in ev_s.zero_shot().items()})
    if ev_oi is not None:
        metrics.update({(f"(oi){k}" if k.startswith("R@") else k): v for k, v in ev_oi.compute().items()})
    if ev_coco is not None:
        metrics["AP50"] = ev_coco.compute()["AP50"]
    if ev_phr is not None:
        metrics.update({f"phrdet_{k}": v for k, v in ev_phr.compute().items()})
    if ev_prd is not None:
        metrics.update({f"preddet_{k}": v for k, v in ev_prd.compute().items()})
    for (name, _, prefix), ev in ev_proto.items():
        res = dict(ev.compute(), **ev.mean_recall())
        if train_counts is not None:
            res.update(ev.zero_shot())
        metrics.update({f"{prefix}{name}_{k}": v for k, v in res.items()})
    return metrics
