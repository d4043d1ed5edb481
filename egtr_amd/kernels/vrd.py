"""Bindings of the phrase- and predicate-detection recall kernels (csrc/vrd_eval.hip).  The caller
(``egtr_amd.evaluation.vrd``) owns the staging; these take the device views of the relation layout
(``evaluation._common.RelationGT``), allocate the outputs and launch one C entry on torch's current stream.
``egtr_amd.ops`` re-exports every name below."""
import ctypes

import torch

from .. import _lib
from .._lib import _chk

__all__ = ["sgg_eval_phrdet", "sgg_eval_preddet", "PREDDET_MAX_GT", "NO_RANK"]

PREDDET_MAX_GT = 1024      # GT relations per image the predicate-detection kernel keeps in LDS (vrd_eval.hip: kMaxGt)
NO_RANK = 0x7fffffff       # first rank of a GT triplet no list entry equals (vrd_eval.hip: kNoRank)


def _width(num_rel, ks):
    return len(ks) + 2 + num_rel * (len(ks) + 1)


def sgg_eval_phrdet(inds, boxes, classes, gt, num_rel, ks, iou_thresh, acc):
    """egtr_sgg_eval_phrdet_f32: ``inds`` int64 [B, K, 3], ``boxes`` float32 [B, N, 4], ``classes`` int64 [B, N], the
    staged ``gt``.  Returns (slab float64 [B, width], first_rank int32 [T]) and adds the slab rows to ``acc`` (may be
    None) in image order."""
    _chk(inds, "pred_rel_inds", torch.int64)
    _chk(boxes, "pred_boxes", torch.float32)
    _chk(classes, "pred_classes", torch.int64)
    B, K, N = inds.shape[0], inds.shape[1], boxes.shape[1]
    slab = torch.empty(B, _width(num_rel, ks), dtype=torch.float64, device=inds.device)
    first_rank = torch.empty(max(gt.T, 1), dtype=torch.int32, device=inds.device)
    _lib.launch("egtr_sgg_eval_phrdet_f32", inds.data_ptr(), inds.shape[2], None, boxes.data_ptr(), classes.data_ptr(), B,
                K, N, int(num_rel), _lib.ptr(gt.rels), gt.rel_off.data_ptr(), int(gt.T), _lib.ptr(gt.boxes),
                _lib.ptr(gt.classes), gt.box_off.data_ptr(), int(gt.G), (ctypes.c_int * len(ks))(*ks), len(ks),
                float(iou_thresh), first_rank.data_ptr(), slab.data_ptr(), _lib.ptr(acc))
    return slab, first_rank[:gt.T]


def sgg_eval_preddet(pairs, scores, gt, ks, acc):
    """egtr_sgg_eval_preddet_f32: ``pairs`` int64 [B, K, 2] (GT object indices), ``scores`` float32 [B, K, R], the staged
    ``gt``.  Returns (slab float64 [B, width], chosen_row, first_rank, first_rank_pred: int32 [T] each) and adds the
    slab rows to ``acc`` (may be None) in image order."""
    _chk(pairs, "pred_rel_inds", torch.int64)
    _chk(scores, "rel_scores", torch.float32)
    B, K, R = scores.shape
    slab = torch.empty(B, _width(R, ks), dtype=torch.float64, device=scores.device)
    out = torch.empty(3, max(gt.T, 1), dtype=torch.int32, device=scores.device)
    _lib.launch("egtr_sgg_eval_preddet_f32", pairs.data_ptr(), scores.data_ptr(), B, K, R, _lib.ptr(gt.rels),
                gt.rel_off.data_ptr(), int(gt.T), gt.box_off.data_ptr(), int(gt.G), (ctypes.c_int * len(ks))(*ks),
                len(ks), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), slab.data_ptr(), _lib.ptr(acc))
    return slab, out[0, :gt.T], out[1, :gt.T], out[2, :gt.T]
