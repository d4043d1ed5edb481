"""Phrase- and predicate-detection recall, the two VRD protocols of the reference's evaluator (lib/evaluation/sg_eval.py:
``BasicSceneGraphEvaluator.vrd_modes()``, the ``phrdet`` / ``preddet`` branches of ``evaluate_from_dict``,
``_compute_pred_matches(phrdet=True)``), accumulated where the model outputs live.  Device tensors go to
``egtr_sgg_eval_phrdet_f32`` / ``egtr_sgg_eval_preddet_f32`` (csrc/vrd_eval.hip); host tensors to the torch
implementations of the same definitions below.  State, slab layout and results are ``SceneGraphRecall``'s.

Phrase detection: a candidate (s, o, p) [K, 3] in rank order matches a GT triplet when both classes and the predicate
agree and the bbox.pyx IoU of the UNION boxes -- (min x1, min y1, max x2, max y2) of subject and object, for the GT and
for the candidate -- is >= ``iou_thresh``.  Everything behind the first ranks (recalls, per-predicate recalls, the
zero-shot pass) is the sgdet evaluator's.

Predicate detection (sg_eval.py:111-132, bug for bug): the candidates are (s, o) PAIRS OF GT OBJECTS [K, 2] with their
predicate scores [K, R].  For GT row j the chosen candidate row is the first whose pair equals the GT pair -- row 0 when
no candidate has it (numpy's argmax of an all-false column).  The image's ranked list holds the n_gt x R entries
(pair of the chosen row of j, p, rel_scores[chosen row of j][p]); GT triplet t is recalled at k when one of the first k
entries equals its (s, o, p).  So a GT pair listed twice (two predicates) contributes every entry twice, and a pair that
fell back to row 0 contributes row 0's entries.  The reference's order is numpy's unstable argsort of the negated
scores; the order is DEFINED here: descending score, NaN last, -0 = +0, ties by ascending flat index j * R + p.  The
per-predicate recalls (mR@k) rank inside the GT rows of that predicate, because the reference's per-predicate evaluators
get a filtered ``gt_relations``.  An image with GT relations and no candidates counts, with recall 0; an image without GT
relations is skipped and counted in ``skipped``.
"""
import torch

from ..kernels.vrd import NO_RANK, PREDDET_MAX_GT, sgg_eval_phrdet, sgg_eval_preddet
from ._common import _MAX_CAND, _bbox_iou_pyx, check_gt_predicates, gt_entry, upload_relation_gt
from .sgg import SceneGraphRecall


# ---- host implementations ---------------------------------------------------------------------------------------------
def _union_boxes(a, b):
    return torch.cat([torch.minimum(a[..., :2], b[..., :2]), torch.maximum(a[..., 2:], b[..., 2:])], -1)


def phrase_first_ranks_host(pred_rels, pred_boxes, pred_classes, gt_rels, gt_boxes, gt_classes, iou_thresh=0.5):
    """``first_ranks_host`` with the phrase-detection box test: int64 [T], K where unmatched."""
    K, T = pred_rels.shape[0], gt_rels.shape[0]
    if K == 0 or T == 0:
        return torch.full((T,), K, dtype=torch.long)
    s, o, p = pred_rels[:, 0], pred_rels[:, 1], pred_rels[:, 2]
    gs, go, gp = gt_rels[:, 0], gt_rels[:, 1], gt_rels[:, 2]
    label = ((pred_classes[s][None, :] == gt_classes[gs][:, None]) & (pred_classes[o][None, :] == gt_classes[go][:, None])
             & (p[None, :] == gp[:, None]))                                                       # [T, K]
    pb, gb = pred_boxes.double(), gt_boxes.double()
    match = label & (_bbox_iou_pyx(_union_boxes(gb[gs], gb[go])[:, None, :],
                                   _union_boxes(pb[s], pb[o])[None, :, :]) >= iou_thresh)
    return torch.where(match, torch.arange(K).expand(T, K), K).min(1).values


def score_keys_host(scores):
    """The order key of float32 scores (int64, same shape): a larger key ranks earlier; NaN is the smallest, -0 = +0
    (``score_key`` of csrc/vrd_eval.hip)."""
    x = scores.float()
    x = torch.where(x == 0, torch.zeros_like(x), x).contiguous()
    u = x.view(torch.int32).long() & 0xFFFFFFFF
    key = torch.where((u & 0x80000000) != 0, ~u & 0xFFFFFFFF, u | 0x80000000)
    return torch.where(x.isnan(), torch.zeros_like(key), key)


def preddet_ranks_host(pairs, scores, gt_rels, num_boxes):
    """The predicate-detection matching of one image on the host.  pairs [K, 2], scores [K, R], gt_rels [T, 3].
    Returns (chosen_row, first_rank, first_rank_pred), int64 [T] each: the chosen candidate row of every GT row; the
    lowest position of an entry equal to the GT triplet in the image's list; the same in the list of the GT rows with
    the triplet's predicate.  NO_RANK where no entry equals it."""
    K, T = pairs.shape[0], gt_rels.shape[0]
    chosen = torch.zeros(T, dtype=torch.long)
    none = torch.full((T,), NO_RANK, dtype=torch.long)
    if K == 0 or T == 0:
        return chosen, none, none.clone()
    R = scores.shape[1]
    pairs, gp = pairs.long(), gt_rels[:, 2]
    cand_ok = ((pairs >= 0) & (pairs < num_boxes)).all(1)
    gt_ok = ((gt_rels[:, :2] >= 0) & (gt_rels[:, :2] < num_boxes)).all(1) & (gp >= 0) & (gp < R)
    prc = (pairs[:, None, :] == gt_rels[None, :, :2]).all(2) & cand_ok[:, None] & gt_ok[None, :]          # [K, T]
    first = torch.where(prc, torch.arange(K)[:, None].expand(K, T), K).min(0).values
    chosen = torch.where(first < K, first, 0)                                      # argmax of an all-false column is 0
    ent_pair = torch.where(cand_ok[chosen][:, None], pairs[chosen], -1)            # [T, 2]
    gt_pair = torch.where(gt_ok[:, None], gt_rels[:, :2], -2)                      # an out-of-range GT row matches nothing
    keys = score_keys_host(scores)[chosen]                                         # [T, R]

    def first_positions(rows):
        k = keys[rows].reshape(-1)
        order = torch.sort(-k, stable=True).indices                   # descending key, ties by ascending flat index
        e_pair, e_p = ent_pair[rows][order // R], order % R           # the ranked list: (pair of the chosen row of j, p)
        hit = (e_pair[:, None, :] == gt_pair[rows][None, :, :]).all(2) & (e_p[:, None] == gp[rows][None, :])   # [L, n]
        pos = torch.arange(k.numel())[:, None].expand_as(hit)
        return torch.where(hit, pos, NO_RANK).min(0).values

    fr = first_positions(torch.arange(T))
    fr_pred = none.clone()
    for q in torch.unique(gp).tolist():
        rows = torch.nonzero(gp == q).flatten()
        fr_pred[rows] = first_positions(rows)
    return chosen, fr, fr_pred


# ---- evaluators ---------------------------------------------------------------------------------------------------------
class _VrdRecall(SceneGraphRecall):
    def merge(self, other):
        if type(other) is not type(self):
            raise ValueError(f"merge needs another {type(self).__name__}")
        return super().merge(other)

    def compute(self):
        """{"R@k", "mR@k"[, "zR@k"]}: the mean per-image recall, the mean over predicates of the per-predicate recalls
        (``per_predicate()`` holds them) and, with ``train_counts``, the zero-shot recall."""
        out = super().compute()
        out.update(self.mean_recall())
        if self._seen_bits is not None:
            out.update(self.zero_shot())
        return out


class PhraseDetectionRecall(_VrdRecall):
    """R@k / mR@k / zR@k of the reference's ``phrdet`` evaluator (``vrd_modes``: multiple predicates per pair, candidates
    [K, 3]): ``SceneGraphRecall`` with the union-box test of the module docstring.  ``train_counts`` as there."""

    def __init__(self, num_rel_labels, ks=(20, 50, 100), iou_thresh=0.5, keep_per_image=False, train_counts=None,
                 train_num_labels=None):
        super().__init__(num_rel_labels, ks=ks, multiple_preds=True, iou_thresh=iou_thresh,
                         keep_per_image=keep_per_image, train_counts=train_counts, train_num_labels=train_num_labels)

    _first_ranks = staticmethod(phrase_first_ranks_host)

    def _launch(self, acc):
        """egtr_sgg_eval_phrdet_f32 on the inputs the last device update staged; returns the slab."""
        inds, _, boxes, classes, gt = self._staged
        with torch.cuda.device(boxes.device):
            slab, self.last_first_rank = sgg_eval_phrdet(inds, boxes, classes, gt, self.num_rel, self.ks,
                                                         self.iou_thresh, acc)
        return slab


class PredicateDetectionRecall(_VrdRecall):
    """R@k / mR@k of the reference's ``preddet`` evaluator (module docstring).  ``update`` takes candidate dicts with
    ``pred_rel_inds`` [K, 2] (pairs of GT object indices; ``runtime.matched_pair_candidates`` builds them from a model's
    outputs) and ``rel_scores`` [K, R].  K may differ between the images of a batch: the device path pads with pairs
    that match nothing, which changes no chosen row.  There is no zero-shot variant (``train_counts`` must be None) and
    no box test (``iou_thresh`` is accepted for a uniform interface and not used).  At most 1024 GT relations per image.
    After a device update ``last_chosen_row`` / ``last_first_rank`` / ``last_first_rank_pred`` hold the kernel's int32
    [T] outputs."""

    def __init__(self, num_rel_labels, ks=(20, 50, 100), iou_thresh=0.5, keep_per_image=False, train_counts=None):
        if train_counts is not None:
            raise ValueError("predicate detection has no zero-shot variant: train_counts must be None")
        super().__init__(num_rel_labels, ks=ks, multiple_preds=True, iou_thresh=iou_thresh,
                         keep_per_image=keep_per_image)

    def update(self, candidates, targets):
        if len(candidates) != len(targets):
            raise ValueError(f"{len(candidates)} candidate entries for {len(targets)} targets")
        if not candidates:
            return
        for c in candidates:
            for key in ("pred_rel_inds", "rel_scores"):
                if key not in c:
                    raise KeyError(f"candidate entry lacks {key!r}")
            inds, rs = c["pred_rel_inds"], c["rel_scores"]
            if inds.dim() != 2 or inds.shape[1] != 2:
                raise ValueError(f"pred_rel_inds must be [K, 2], got {tuple(inds.shape)}")
            if inds.shape[0] > _MAX_CAND:
                raise ValueError(f"at most {_MAX_CAND} candidates per image, got {inds.shape[0]}")
            if rs.dim() != 2 or rs.shape[0] != inds.shape[0] or rs.shape[1] != self.num_rel:
                raise ValueError(f"rel_scores must be [K, {self.num_rel}], got {tuple(rs.shape)}")
        gts = [gt_entry(t) for t in targets]
        for g in gts:
            check_gt_predicates(g, self.num_rel)
            if g["gt_relations"].shape[0] > PREDDET_MAX_GT:
                raise ValueError(f"at most {PREDDET_MAX_GT} GT relations per image, got {g['gt_relations'].shape[0]}")
        device = candidates[0]["pred_rel_inds"].device
        if device.type == "cpu":
            self._update_host(candidates, gts)
        else:
            self._update_device(candidates, gts, device)

    def _image_row(self, fr, fr_pred, gt_rels):
        """One slab row (float64 [W]) from the two first ranks of an image, as the kernel writes it."""
        nk, R = len(self.ks), self.num_rel
        row = torch.zeros(self.width, dtype=torch.float64)
        T = gt_rels.shape[0]
        if T == 0:
            row[nk + 1] = 1.0
            return row
        row[:nk] = torch.tensor([float(int((fr < k).sum())) / float(T) for k in self.ks], dtype=torch.float64)
        row[nk] = 1.0
        p = gt_rels[:, 2]
        cnt = torch.bincount(p, minlength=R)
        hits_p = torch.zeros(R, nk, dtype=torch.long).index_add_(0, p, torch.stack([fr_pred < k for k in self.ks], 1).long())
        for q in torch.nonzero(cnt).flatten().tolist():
            n = float(cnt[q])
            row[self._pbase + q * nk: self._pbase + (q + 1) * nk] = torch.tensor(
                [float(h) / n for h in hits_p[q].tolist()], dtype=torch.float64)
            row[self._fbase + q] = 1.0
        return row

    def _update_host(self, candidates, gts):
        acc = self._acc_on(torch.device("cpu"))
        rows, outs = [], []
        for c, g in zip(candidates, gts):
            out = preddet_ranks_host(c["pred_rel_inds"], c["rel_scores"].float(), g["gt_relations"],
                                     g["gt_classes"].shape[0])
            outs.append(out)
            rows.append(self._image_row(out[1], out[2], g["gt_relations"]))
        for r in rows:          # image order, like the fold launch
            acc.add_(r)
        self.last_chosen_row, self.last_first_rank, self.last_first_rank_pred = (
            torch.cat([o[i] for o in outs]) for i in range(3))
        if self.keep_per_image:
            self._per_image.append(torch.stack(rows)[:, :len(self.ks) + 2])

    def _update_device(self, candidates, gts, device):
        acc = self._acc_on(device)
        B, K = len(candidates), max(c["pred_rel_inds"].shape[0] for c in candidates)
        pairs = torch.full((B, K, 2), -1, dtype=torch.long, device=device)      # (-1, -1): matches no GT pair
        scores = torch.zeros(B, K, self.num_rel, dtype=torch.float32, device=device)
        for b, c in enumerate(candidates):
            k = c["pred_rel_inds"].shape[0]
            pairs[b, :k] = c["pred_rel_inds"]
            scores[b, :k] = c["rel_scores"]
        gt = upload_relation_gt(self._ring, gts, device)
        self._staged = (pairs, scores, gt)
        with torch.cuda.device(device):
            slab, self.last_chosen_row, self.last_first_rank, self.last_first_rank_pred = sgg_eval_preddet(
                pairs, scores, gt, self.ks, acc)
        if self.keep_per_image:
            self._per_image.append(slab[:, :len(self.ks) + 2].clone())
