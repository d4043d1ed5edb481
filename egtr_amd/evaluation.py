"""Scene-graph Recall@K and mean Recall@K (the reference's sgdet evaluator, lib/evaluation/sg_eval.py, as driven by
evaluate_batch / evaluate, train_egtr.py:43-139 and evaluate_egtr.py:40-127), accumulated where the model outputs live.

One matching pass per image gives every metric: for each GT triplet, its FIRST MATCHING RANK (the smallest candidate index
whose subject / object classes and predicate agree and whose subject and object boxes both have bbox.pyx IoU >= 0.5 with
the GT's; the candidate count if none).  The reference's ``len(reduce(np.union1d, pred_to_gt[:k]))`` is the number of GT
triplets whose first rank is < k, and its per-predicate evaluators (the GT list filtered by predicate) see the same
first ranks.  Device tensors go to ``egtr_sgg_eval_f32`` (csrc/sgg_eval.hip); host tensors to a vectorised torch
implementation of the same matching (``first_ranks_host``), so the API also runs without a GPU.

Differences from the reference, on purpose:
  * an image without GT relations is skipped and counted in ``skipped`` (sg_eval.py:199 raises an AssertionError);
  * R@k averages are accumulated as a left fold in image order (deterministic, batch-size independent); numpy's mean
    sums pairwise, so the metrics agree to ~1e-15, while the per-image recalls are bit-identical.
The Open Images branch (``OpenImagesRelationMetrics``; oi_eval.py eval_rel_results, ap_eval_rel.py; csrc/oi_eval.hip)
reproduces these reference semantics:
  * every (subject, object) pair is a candidate, self pairs included; pred_scores = clamp(pred_rel) * clamp(connectivity);
  * per pair the prd_k = 2 best predicates (np.argsort(-row)); spo = (s_sbj * s_obj) * top_j, two float32 roundings; the
    topk = 100 largest entries of the pair-major [M, 2] array, of which only those > 1e-5 are kept (NaN is dropped);
  * recall: _compute_pred_matches with labels (s, p, o) and the fp64 bbox.pyx IoU (+1, >= 0.5) at k in (1, 5, 10, 20, 50,
    100); per image hits / (n_gt + 1e-12), micro sum(hits) / (sum(n_gt) + 1e-12);
  * AP per predicate class over all images' detections sorted by confidence: greedy VOC assignment with the float32
    ap_eval_rel.bbox_iou (intersection (min - max) + 1 clamped at 0, areas WITHOUT +1) times the label mask, jmax the
    first argmax, TP iff ovmax > 0.5 (strict) and jmax not yet visited (no fall-back to another GT); rel mode
    min(iou_s, iou_o), phr mode the union boxes; rec = cumsum(tp) / (npos + 1e-12), prec = tp / max(tp + fp, eps),
    get_ap's all-point interpolation; AP = 0 for a class without detections or without GT;
  * rel_mAP = sum AP / C, w_rel_mAP = sum AP * npos_c / sum npos (class order; the same for phr);
    score = 0.4 * w_rel + 0.4 * w_phr + 0.2 * microR@50.
Tie rules the reference leaves to numpy's quicksort, defined here: equal predicate scores rank by lower predicate index;
equal spo by lower flat index; equal confidences of one class by image order, then in-image rank.  An image without GT
relations is skipped and counted (the reference raises a KeyError).
The COCO box-detection metrics (``CocoDetectionMetrics``; pycocotools COCOeval(iouType="bbox") as the reference's
CocoEvaluator runs it, lib/evaluation/coco_eval.py; csrc/coco_eval.hip) reproduce evaluateImg's greedy matching at ten
IoU thresholds and four area ranges, accumulate's precision / recall tables and summarize's 12 stats.  Image order is
update order (the reference sorts by image id); a match is a flag, not a GT id (pycocotools ignores a match to a GT whose
annotation id is 0); ``evaluate(coco=True)`` adds the reference's "AP50".
"""
import ctypes
import math
import types

import numpy as np
import torch

from . import _lib

_MAX_CAND, _MAX_REL, _MAX_K = 1024, 256, 8


def rescale_bboxes(boxes, orig_size):
    """util/box_ops.py:87-91 for a target: normalised cxcywh -> xyxy, then x (w, h, w, h) in float32.
    ``orig_size`` is (h, w) like the targets' ``orig_size``."""
    h, w = orig_size[0], orig_size[1]
    cx, cy, bw, bh = boxes.unbind(-1)
    b = torch.stack([(cx - 0.5 * bw), (cy - 0.5 * bh), (cx + 0.5 * bw), (cy + 0.5 * bh)], dim=-1)
    return b * torch.tensor([w, h, w, h], dtype=torch.float32)


def gt_entry(target):
    """The reference's ``gt_entry`` of one target dict (train_egtr.py:69-80), on the host."""
    t = {k: (v.cpu() if torch.is_tensor(v) else torch.as_tensor(v)) for k, v in target.items()}
    return {"gt_relations": t["rel"].nonzero(),
            "gt_boxes": rescale_bboxes(t["boxes"].float(), t["orig_size"]),
            "gt_classes": t["class_labels"].long()}


def _bbox_iou_pyx(gt, q):
    """bbox.pyx bbox_overlaps (:21-61) between paired rows of gt [..., 4] and q [..., 4] (float64), the same operation
    order as the Cython loop (every torch op rounds: no contraction)."""
    box_area = (q[..., 2] - q[..., 0] + 1) * (q[..., 3] - q[..., 1] + 1)
    iw = torch.minimum(gt[..., 2], q[..., 2]) - torch.maximum(gt[..., 0], q[..., 0]) + 1
    ih = torch.minimum(gt[..., 3], q[..., 3]) - torch.maximum(gt[..., 1], q[..., 1]) + 1
    ua = (gt[..., 2] - gt[..., 0] + 1) * (gt[..., 3] - gt[..., 1] + 1) + box_area - iw * ih
    iou = iw * ih / ua
    return torch.where((iw > 0) & (ih > 0), iou, torch.zeros((), dtype=torch.float64))


def numpy_argmax(rows):
    """numpy ``argmax(1)`` of a float tensor [K, R]: the lowest index among the maxima, the first NaN if any."""
    R = rows.shape[1]
    idx = torch.arange(R, device=rows.device).expand_as(rows)
    nan = rows.isnan()
    first_nan = torch.where(nan, idx, R).min(1).values
    top = rows.masked_fill(nan, float("-inf")).max(1, keepdim=True).values
    first_max = torch.where(rows == top, idx, R).min(1).values
    return torch.where(nan.any(1), first_nan, first_max.clamp(max=R - 1))


def first_ranks_host(pred_rels, pred_boxes, pred_classes, gt_rels, gt_boxes, gt_classes, iou_thresh=0.5):
    """First matching rank of each GT triplet (host, vectorised).  pred_rels [K, 3] (s, o, p) in rank order, pred_boxes
    [N, 4], pred_classes [N], gt_rels [T, 3], gt_boxes [G, 4], gt_classes [G].  Returns int64 [T], K where unmatched."""
    K, T = pred_rels.shape[0], gt_rels.shape[0]
    if K == 0 or T == 0:
        return torch.full((T,), K, dtype=torch.long)
    s, o, p = pred_rels[:, 0], pred_rels[:, 1], pred_rels[:, 2]
    gs, go, gp = gt_rels[:, 0], gt_rels[:, 1], gt_rels[:, 2]
    label = ((pred_classes[s][None, :] == gt_classes[gs][:, None]) & (pred_classes[o][None, :] == gt_classes[go][:, None])
             & (p[None, :] == gp[:, None]))                                                       # [T, K]
    pb, gb = pred_boxes.double(), gt_boxes.double()
    sub = _bbox_iou_pyx(gb[gs][:, None, :], pb[s][None, :, :]) >= iou_thresh
    obj = _bbox_iou_pyx(gb[go][:, None, :], pb[o][None, :, :]) >= iou_thresh
    match = label & sub & obj
    ranks = torch.arange(K).expand(T, K)
    return torch.where(match, ranks, K).min(1).values


def _check_candidate(c, multiple, num_rel):
    for key in ("pred_boxes", "pred_classes", "pred_rel_inds") + (() if multiple else ("rel_scores",)):
        if key not in c:
            raise KeyError(f"candidate entry lacks {key!r}")
    inds = c["pred_rel_inds"]
    if inds.dim() != 2 or inds.shape[1] < (3 if multiple else 2):
        raise ValueError(f"pred_rel_inds must be [K, {3 if multiple else 2}], got {tuple(inds.shape)}")
    if inds.shape[0] > _MAX_CAND:
        raise ValueError(f"at most {_MAX_CAND} candidates per image, got {inds.shape[0]}")
    if not multiple:
        rs = c["rel_scores"]
        if rs.dim() != 2 or rs.shape[0] != inds.shape[0] or rs.shape[1] != num_rel:
            raise ValueError(f"rel_scores must be [K, {num_rel}] in single-predicate mode, got {tuple(rs.shape)}")


class SceneGraphRecall:
    """R@k (and per-predicate R@k, mR@k) of the reference's BasicSceneGraphEvaluator in sgdet mode.

    ``multiple_preds=False``: graph-constrained (the reference's "single" evaluator: candidates [K, 2] + rel_scores
    [K, R], predicate = argmax of the row); ``True``: candidates [K, 3].  All metrics live in ONE flat float64 tensor
    ``acc`` (sums of per-image recalls, image counts, skipped count; see csrc/sgg_eval.hip for the layout), on the device
    of the first ``update`` -- ``merge`` / ``all_reduce`` add it."""

    def __init__(self, num_rel_labels, ks=(20, 50, 100), multiple_preds=False, iou_thresh=0.5, keep_per_image=False):
        ks = tuple(int(k) for k in ks)
        if not 1 <= num_rel_labels <= _MAX_REL:
            raise ValueError(f"num_rel_labels must be in [1, {_MAX_REL}], got {num_rel_labels}")
        if not 1 <= len(ks) <= _MAX_K or any(k < 1 for k in ks) or any(b <= a for a, b in zip(ks, ks[1:])):
            raise ValueError(f"ks must be 1..{_MAX_K} ascending positive values, got {ks}")
        if not math.isfinite(iou_thresh):
            raise ValueError("iou_thresh must be finite")
        self.num_rel = int(num_rel_labels)
        self.ks = ks
        self.multiple_preds = bool(multiple_preds)
        self.iou_thresh = float(iou_thresh)
        self.keep_per_image = bool(keep_per_image)
        nk, R = len(ks), self.num_rel
        self.width = nk + 2 + R * (nk + 1)
        self._pbase, self._fbase = nk + 2, nk + 2 + R * nk
        self._ring = []            # [pinned buffer, event] staging slots of the host -> device GT copies
        self.reset()

    # ---- state -----------------------------------------------------------------------------------------------------
    def reset(self, device=None):
        self.acc = None if device is None else torch.zeros(self.width, dtype=torch.float64, device=device)
        self._per_image = []       # slab columns [B, nk + 2] (recalls, counted, skipped) per update

    def _acc_on(self, device):
        if self.acc is None:
            self.acc = torch.zeros(self.width, dtype=torch.float64, device=device)
        elif self.acc.device != device:
            raise ValueError(f"this evaluator accumulates on {self.acc.device}, got inputs on {device}")
        return self.acc

    def merge(self, other):
        """Add another evaluator's accumulators (same ks / num_rel_labels) into this one."""
        if (other.ks, other.num_rel, other.multiple_preds) != (self.ks, self.num_rel, self.multiple_preds):
            raise ValueError("merge needs evaluators with the same ks, num_rel_labels and mode")
        if other.acc is not None:
            self._acc_on(other.acc.device).add_(other.acc)
        self._per_image += other._per_image
        return self

    def all_reduce(self, group=None):
        """Sum the accumulators over the ranks of ``group`` (one collective on the flat tensor).  No-op when
        torch.distributed is not initialised."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return self
        if self.acc is None:
            self.acc = torch.zeros(self.width, dtype=torch.float64,
                                   device="cuda" if dist.get_backend(group) == "nccl" else "cpu")
        dist.all_reduce(self.acc, op=dist.ReduceOp.SUM, group=group)
        return self

    # ---- update ----------------------------------------------------------------------------------------------------
    def update(self, candidates, targets):
        """Score one batch.  ``candidates``: ``runtime.triplet_candidates`` output (or dicts with the reference's
        ``pred_entry`` keys); ``targets``: the reference's target dicts (class_labels, normalised cxcywh boxes, dense rel
        [n, n, R], orig_size (h, w)), on the host.  On the device path nothing is copied back and nothing waits."""
        if len(candidates) != len(targets):
            raise ValueError(f"{len(candidates)} candidate entries for {len(targets)} targets")
        if not candidates:
            return
        for c in candidates:
            _check_candidate(c, self.multiple_preds, self.num_rel)
        if len({c["pred_rel_inds"].shape[0] for c in candidates}) != 1:
            raise ValueError("every image of a batch needs the same number of candidates")
        if len({c["pred_boxes"].shape[0] for c in candidates}) != 1:
            raise ValueError("every image of a batch needs the same number of predicted boxes")
        gts = [gt_entry(t) for t in targets]
        for g in gts:
            if g["gt_relations"].numel() and int(g["gt_relations"][:, 2].max()) >= self.num_rel:
                raise ValueError(f"a GT predicate is outside [0, {self.num_rel})")
        device = candidates[0]["pred_rel_inds"].device
        if device.type == "cpu":
            self._update_host(candidates, gts)
        else:
            self._update_device(candidates, gts, device)

    def _image_row(self, fr, gt_rels, K):
        """One slab row (float64 [W]) from the first ranks of an image, as the kernel writes it."""
        nk, R = len(self.ks), self.num_rel
        row = torch.zeros(self.width, dtype=torch.float64)
        T = gt_rels.shape[0]
        if T == 0:
            row[nk + 1] = 1.0
            return row
        hit = torch.stack([fr < min(k, K) for k in self.ks], 1)                              # [T, nk]
        row[:nk] = torch.tensor([float(h) / float(T) for h in hit.sum(0).tolist()], dtype=torch.float64)
        row[nk] = 1.0
        p = gt_rels[:, 2]
        cnt = torch.bincount(p, minlength=R)
        hits_p = torch.zeros(R, nk, dtype=torch.long).index_add_(0, p, hit.long())
        for q in torch.nonzero(cnt).flatten().tolist():
            n = float(cnt[q])
            row[self._pbase + q * nk: self._pbase + (q + 1) * nk] = torch.tensor(
                [float(h) / n for h in hits_p[q].tolist()], dtype=torch.float64)
            row[self._fbase + q] = 1.0
        return row

    def _update_host(self, candidates, gts):
        acc = self._acc_on(torch.device("cpu"))
        rows = []
        for c, g in zip(candidates, gts):
            inds = c["pred_rel_inds"].long()
            if self.multiple_preds:
                rels = inds[:, :3]
            else:
                rels = torch.cat([inds[:, :2], numpy_argmax(c["rel_scores"].float())[:, None]], 1)
            fr = first_ranks_host(rels, c["pred_boxes"].float(), c["pred_classes"].long(), g["gt_relations"],
                                  g["gt_boxes"], g["gt_classes"], self.iou_thresh)
            rows.append(self._image_row(fr, g["gt_relations"], rels.shape[0]))
        for r in rows:          # image order, like sgg_fold
            acc.add_(r)
        if self.keep_per_image:
            self._per_image.append(torch.stack(rows)[:, :len(self.ks) + 2])

    def _stage(self, nbytes):
        """A pinned staging buffer no in-flight copy still reads: a slot whose event has completed is reused, otherwise
        a new slot is added (event.query() never waits)."""
        for slot in self._ring:
            if slot[0].numel() >= nbytes and slot[1].query():
                return slot
        slot = [torch.empty(max(nbytes, 4096), dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
        self._ring.append(slot)
        if len(self._ring) > 8:   # drop a finished slot so the ring stays small
            for i, s in enumerate(self._ring[:-1]):
                if s[1].query():
                    del self._ring[i]
                    break
        return slot

    def _update_device(self, candidates, gts, device):
        acc = self._acc_on(device)
        B = len(candidates)

        def stacked(key, dtype):
            ts = [c[key] for c in candidates]
            x = ts[0].unsqueeze(0) if B == 1 else torch.stack(ts)
            return x.to(dtype).contiguous()

        inds = stacked("pred_rel_inds", torch.long)
        cols = 3 if self.multiple_preds else 2
        if inds.shape[2] != cols:
            inds = inds[:, :, :cols].contiguous()
        scores = None if self.multiple_preds else stacked("rel_scores", torch.float32)
        boxes = stacked("pred_boxes", torch.float32)
        classes = stacked("pred_classes", torch.long)
        # ragged GT packed into one pinned buffer: int64 [rel_off B+1 | box_off B+1 | rels 3T | classes G], float32 boxes 4G
        rels = [g["gt_relations"] for g in gts]
        T = sum(r.shape[0] for r in rels)
        G = sum(g["gt_classes"].shape[0] for g in gts)
        n64 = 2 * (B + 1) + 3 * T + G
        nbytes = 8 * n64 + 16 * G
        buf, ev = self._stage(nbytes)
        i64 = buf[:8 * n64].view(torch.int64)
        f32 = buf[8 * n64:nbytes].view(torch.float32)
        rel_off = torch.tensor([0] + [r.shape[0] for r in rels], dtype=torch.int64).cumsum(0)
        box_off = torch.tensor([0] + [g["gt_classes"].shape[0] for g in gts], dtype=torch.int64).cumsum(0)
        i64[:B + 1] = rel_off
        i64[B + 1:2 * B + 2] = box_off
        if T:
            i64[2 * B + 2:2 * B + 2 + 3 * T] = torch.cat(rels).reshape(-1)
        if G:
            i64[2 * B + 2 + 3 * T:] = torch.cat([g["gt_classes"] for g in gts])
            f32.copy_(torch.cat([g["gt_boxes"] for g in gts]).reshape(-1))
        dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        dev.copy_(buf[:nbytes], non_blocking=True)
        ev.record()
        self._staged = (inds, scores, boxes, classes, dev, B, T, G)
        slab = self._launch(acc)
        if self.keep_per_image:
            self._per_image.append(slab[:, :len(self.ks) + 2].clone())

    def _launch(self, acc):
        """egtr_sgg_eval_f32 on the inputs the last device update staged (``_staged``); returns the slab."""
        inds, scores, boxes, classes, dev, B, T, G = self._staged
        K, N = inds.shape[1], boxes.shape[1]
        n64 = 2 * (B + 1) + 3 * T + G
        d64 = dev[:8 * n64].view(torch.int64)
        d_boxes = dev[8 * n64:].view(torch.float32)
        slab = torch.empty(B, self.width, dtype=torch.float64, device=dev.device)
        first_rank = torch.empty(max(T, 1), dtype=torch.int32, device=dev.device)
        ks = (ctypes.c_int * len(self.ks))(*self.ks)
        stream = torch.cuda.current_stream(dev.device).cuda_stream
        _lib.check(_lib.lib().egtr_sgg_eval_f32(
            stream, inds.data_ptr(), inds.shape[2], _lib.ptr(scores), boxes.data_ptr(),
            classes.data_ptr(), B, K, N, self.num_rel, d64[2 * B + 2:].data_ptr() if T else None, d64.data_ptr(), T,
            d_boxes.data_ptr() if G else None, d64[2 * B + 2 + 3 * T:].data_ptr() if G else None,
            d64[B + 1:].data_ptr(), G, ks, len(self.ks), self.iou_thresh, first_rank.data_ptr(), slab.data_ptr(),
            _lib.ptr(acc)), "egtr_sgg_eval_f32")
        self.last_first_rank = first_rank[:T]
        return slab

    # ---- results (one synchronisation each) --------------------------------------------------------------------------
    def _host_acc(self):
        if self.acc is None:
            return torch.zeros(self.width, dtype=torch.float64)
        return self.acc.cpu()

    @staticmethod
    def _mean(s, n):
        return s / n if n > 0 else float("nan")   # np.mean([]) is nan

    def compute(self):
        """{"R@k": mean per-image recall} over the images seen (the reference's print_stats)."""
        a = self._host_acc().tolist()
        nk = len(self.ks)
        return {f"R@{k}": self._mean(a[j], a[nk]) for j, k in enumerate(self.ks)}

    @property
    def n_images(self):
        return int(self._host_acc()[len(self.ks)])

    @property
    def skipped(self):
        return int(self._host_acc()[len(self.ks) + 1])

    def per_predicate(self):
        """{p: {"R@k": ...}} for every predicate index p; NaN where no image had a GT triplet of p."""
        a = self._host_acc().tolist()
        nk = len(self.ks)
        out = {}
        for p in range(self.num_rel):
            n = a[self._fbase + p]
            out[p] = {f"R@{k}": self._mean(a[self._pbase + p * nk + j], n) for j, k in enumerate(self.ks)}
        return out

    def mean_recall(self):
        """{"mR@k": ...}: calculate_mR_from_evaluator_list (sg_eval.py:316-356) -- predicates with a NaN recall (seen in no
        image) are left out of the sum, but the sum is still divided by the number of predicates."""
        per = self.per_predicate()
        last = f"R@{self.ks[-1]}"
        out = {}
        for k in self.ks:
            s = 0.0
            for v in per.values():
                if math.isnan(v[last]):
                    continue
                s += v[f"R@{k}"]
            out[f"mR@{k}"] = s / self.num_rel
        return out

    def per_image(self):
        """Per-image recalls [n_images, len(ks)] (float64, host) of the images that were not skipped, in update order."""
        if not self.keep_per_image:
            raise RuntimeError("construct the evaluator with keep_per_image=True")
        nk = len(self.ks)
        if not self._per_image:
            return torch.zeros(0, nk, dtype=torch.float64)
        rows = torch.cat([r.cpu() for r in self._per_image])
        return rows[rows[:, nk + 1] == 0][:, :nk]



@torch.no_grad()
def evaluate(model, batches, num_labels, num_rel_labels, single=True, multiple=False, max_topk=100, graphed=True,
             forward=None, oi=False, coco=False, feature_extractor=None):
    """The Visual Genome path of the reference's ``evaluate`` (evaluate_egtr.py:40-127): run the model over ``batches``
    (the reference's collate_fn format: pixel_values, pixel_mask, labels), build the candidates on the device
    (``runtime.triplet_candidates``) and score them.  Returns the reference's ``metric_dict`` keys: ``R@k`` / ``mR@k``
    of the multiple-predicate evaluator and ``(single)R@k`` / ``(single)mR@k`` of the single-predicate one.  The
    model runs through a ``GraphedForward`` when ``graphed`` (and a GPU is present); one created here is released before
    returning (``forward``: an existing ``GraphedForward`` to reuse instead, left as it is).  ``oi``: also score the
    Open Images branch (``OpenImagesRelationMetrics`` on ``triplet_candidates(mode="oi")``) and add its keys --
    w_rel_mAP, w_phr_mAP, microR@50, score, rel_mAP, phr_mAP, microR@k, and the per-image mean recalls as (oi)R@k.
    ``coco``: also score the boxes (``feature_extractor.post_process`` with the targets' orig_size, default a
    ``DeformableDetrFeatureExtractor``, into ``CocoDetectionMetrics(num_labels)``) and add the reference's "AP50"."""
    from .runtime import GraphedForward, triplet_candidates
    if not (single or multiple or oi or coco):
        raise ValueError("enable at least one of single / multiple / oi / coco")
    model.eval()
    device = next(model.parameters()).device
    ev_s = SceneGraphRecall(num_rel_labels, multiple_preds=False) if single else None
    ev_m = SceneGraphRecall(num_rel_labels, multiple_preds=True) if multiple else None
    ev_oi = OpenImagesRelationMetrics(num_rel_labels) if oi else None
    ev_coco = CocoDetectionMetrics(num_labels) if coco else None
    if coco and feature_extractor is None:
        from .feature_extraction import DeformableDetrFeatureExtractor
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
            if ev_m is not None:
                ev_m.update(triplet_candidates(outputs, num_labels, sizes, max_topk, mode="multiple"), targets)
            if ev_s is not None:
                ev_s.update(triplet_candidates(outputs, num_labels, sizes, max_topk, mode="single"), targets)
            if ev_oi is not None:
                ev_oi.update(triplet_candidates(outputs, num_labels, sizes, max_topk, mode="oi"), targets)
            if ev_coco is not None:
                boxes_out = types.SimpleNamespace(logits=outputs["logits"], pred_boxes=outputs["pred_boxes"])
                ev_coco.update(feature_extractor.post_process(boxes_out, sizes), targets)
    finally:
        if own:
            for h in fwd._hooks:
                h.remove()
            fwd._hooks.clear()
            fwd._drop_all()
    metrics = {}
    if ev_m is not None:
        metrics.update(ev_m.compute())
        metrics.update(ev_m.mean_recall())
    if ev_s is not None:
        metrics.update({f"(single){k}": v for k, v in ev_s.compute().items()})
        metrics.update({f"(single){k}": v for k, v in ev_s.mean_recall().items()})
    if ev_oi is not None:
        metrics.update({(f"(oi){k}" if k.startswith("R@") else k): v for k, v in ev_oi.compute().items()})
    if ev_coco is not None:
        metrics["AP50"] = ev_coco.compute()["AP50"]
    return metrics


# ---- Open Images relation metrics ---------------------------------------------------------------------------------------
_OI_MAX_PAIRS, _OI_MAX_TOPK, _OI_MAX_PRDK, _OI_MAX_GT = 300 * 300, 1024, 8, 4096


def bbox_iou_f32(a, b):
    """ap_eval_rel.bbox_iou between broadcast rows of a [..., 4] and b [..., 4] (float32): the intersection is
    ``(min - max) + 1`` clamped at 0, the areas have NO +1, the result is ``inter / ((area_a + area_b) - inter)``."""
    lt = torch.maximum(a[..., :2], b[..., :2])
    rb = torch.minimum(a[..., 2:], b[..., 2:])
    wh = (rb - lt + 1).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    return inter / (area_a + area_b - inter)


def _union(s, o):
    """ap_eval_rel.boxes_union of paired rows."""
    return torch.cat([torch.minimum(s[..., :2], o[..., :2]), torch.maximum(s[..., 2:], o[..., 2:])], -1)


def oi_select_host(pred_scores, obj_scores, pairs, topk=100, prd_k=2):
    """The detection selection of eval_rel_results (oi_eval.py:102-160) for one image, on the host.  pred_scores [M, R]
    float32, obj_scores [N], pairs [M, 2] (s, o).  Every pair keeps its kk = min(prd_k, R) best predicates (NaN last,
    equal scores to the lower predicate index); spo = (score_s * score_o) * top_j in float32; the ``topk`` largest
    entries > 1e-5 by score, ties to the lower flat index m * kk + j.  Returns (sop int64 [K, 3] (s, o, p), score [K])."""
    R = pred_scores.shape[1]
    kk = min(prd_k, R)
    neg, labels = torch.sort(-pred_scores, dim=1, stable=True)          # ascending: NaN last, ties by index
    top = -neg[:, :kk]
    so = obj_scores[pairs[:, 0]] * obj_scores[pairs[:, 1]]
    spo = (so[:, None] * top).reshape(-1)
    keep = torch.nonzero(spo > 1e-5).flatten()
    order = torch.sort(-spo[keep], stable=True).indices[:topk]
    sel = keep[order]
    m, j = sel // kk, sel % kk
    sop = torch.stack([pairs[m, 0], pairs[m, 1], labels[m, j]], 1).long()
    return sop, spo[sel]


def oi_tp_host(sop, pred_boxes, pred_classes, gt_rels, gt_boxes, gt_classes):
    """TP flags of one image's detections (rank order) for ap_eval in rel and phr mode: bool [2, K].  Per predicate
    class, the greedy VOC assignment of ap_eval_rel.ap_eval: overlaps with the class's GT triplets times the label mask,
    ovmax = torch.max (NaN if any NaN), jmax = first argmax; TP when ovmax > 0.5 and jmax is not yet visited."""
    K = sop.shape[0]
    tp = torch.zeros(2, K, dtype=torch.bool)
    if K == 0 or gt_rels.shape[0] == 0:
        return tp
    s, o, p = sop[:, 0], sop[:, 1], sop[:, 2]
    ds, do = pred_boxes[s].float(), pred_boxes[o].float()
    gs, go, gp = gt_rels[:, 0], gt_rels[:, 1], gt_rels[:, 2]
    gsb, gob = gt_boxes[gs].float(), gt_boxes[go].float()
    valid = (gt_classes[gs][None, :] == pred_classes[s][:, None]) & (gt_classes[go][None, :] == pred_classes[o][:, None])
    m = valid.float()
    ov_rel = torch.minimum(bbox_iou_f32(ds[:, None], gsb[None]), bbox_iou_f32(do[:, None], gob[None])) * m
    ov_phr = bbox_iou_f32(_union(ds, do)[:, None], _union(gsb, gob)[None]) * m
    same = gp[None, :] == p[:, None]
    visited = [set(), set()]
    for d in range(K):
        cols = torch.nonzero(same[d]).flatten()
        if cols.numel() == 0 or not bool(valid[d, cols].any()):
            continue
        for mode, ov in enumerate((ov_rel, ov_phr)):
            row = ov[d, cols]
            if bool(row.isnan().any()):
                continue
            mx = row.max()
            if not bool(mx > 0.5):
                continue
            j = int(cols[int(torch.nonzero(row == mx)[0])])
            if j not in visited[mode]:
                visited[mode].add(j)
                tp[mode, d] = True
    return tp


def oi_ap_host(tp, n, npos):
    """get_ap of ap_eval over one class's TP flags (bool [n], confidence order): fp64, the area as a left fold in record
    order -- the same terms and order as the oi_ap kernel."""
    if n == 0:
        return 0.0
    cum = torch.cumsum(tp.to(torch.int64), 0).double()
    prec = cum / torch.arange(1, n + 1, dtype=torch.float64)
    env = torch.flip(torch.cummax(torch.flip(prec, [0]), 0).values, [0]).clamp(min=0.0)
    rec = cum / (float(npos) + 1e-12)
    prev = torch.cat([torch.zeros(1, dtype=torch.float64), rec[:-1]])
    ap = 0.0
    for t in ((rec - prev) * env).tolist():
        if t != 0.0:
            ap += t
    return ap


def _tensor(x):
    return x if torch.is_tensor(x) else torch.as_tensor(x)


class OpenImagesRelationMetrics:
    """Relation metrics of the reference's Open Images evaluator (OIEvaluator.aggregate_metrics without the COCO
    detection part): w_rel_mAP, w_phr_mAP, microR@50, score, rel_mAP, phr_mAP, micro and per-image mean R@k.

    ``update`` takes ``runtime.triplet_candidates(mode="oi")`` output (or dicts with the reference's OI ``pred_entry``
    keys) plus the reference's target dicts.  Device tensors go to the HIP kernels of csrc/oi_eval.hip without a host
    synchronisation; host tensors to a torch implementation of the same semantics.  Per batch the recall counts and npos
    go into one flat float64 accumulator ``acc`` (layout in oi_eval.hip) and every detection leaves a record (predicate,
    score, TP flag in rel and phr mode); ``compute`` sorts the records by class and confidence once and scores the AP.

    Defined where the reference leaves it open: equal predicate scores rank by lower predicate index; equal spo scores by
    lower flat index (pair-major); equal confidences of one class by image order, then in-image rank.  An image without GT
    relations is skipped and counted in ``skipped`` (the reference raises a KeyError)."""

    def __init__(self, num_rel_labels, ks=(1, 5, 10, 20, 50, 100), topk=100, prd_k=2):
        ks = tuple(int(k) for k in ks)
        if not 1 <= num_rel_labels <= _MAX_REL:
            raise ValueError(f"num_rel_labels must be in [1, {_MAX_REL}], got {num_rel_labels}")
        if not 1 <= len(ks) <= _MAX_K or any(k < 1 for k in ks) or any(b <= a for a, b in zip(ks, ks[1:])):
            raise ValueError(f"ks must be 1..{_MAX_K} ascending positive values, got {ks}")
        if not 1 <= topk <= _OI_MAX_TOPK:
            raise ValueError(f"topk must be in [1, {_OI_MAX_TOPK}], got {topk}")
        if not 1 <= prd_k <= _OI_MAX_PRDK:
            raise ValueError(f"prd_k must be in [1, {_OI_MAX_PRDK}], got {prd_k}")
        self.num_rel = int(num_rel_labels)
        self.ks = ks
        self.topk = int(topk)
        self.prd_k = int(prd_k)
        nk = len(ks)
        self.width = 2 * nk + 3 + self.num_rel
        self._ring = []            # [pinned buffer, event] staging slots of the host -> device GT copies
        self.reset()

    # ---- state -----------------------------------------------------------------------------------------------------
    def reset(self, device=None):
        self.acc = None if device is None else torch.zeros(self.width, dtype=torch.float64, device=device)
        self._batches = []         # (p [B, topk], score [B, topk], tp uint8 [2, B, topk], valid bool [B, topk]) per update

    def _acc_on(self, device):
        if self.acc is None:
            self.acc = torch.zeros(self.width, dtype=torch.float64, device=device)
        elif self.acc.device != device:
            raise ValueError(f"this evaluator accumulates on {self.acc.device}, got inputs on {device}")
        return self.acc

    def _records(self):
        """Flat detection records in image order: (p int64 [n], score float32 [n], tp uint8 [2, n])."""
        dev = self.acc.device if self.acc is not None else torch.device("cpu")
        if not self._batches:
            return (torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.float32, device=dev),
                    torch.zeros(2, 0, dtype=torch.uint8, device=dev))
        ps, ss, ts = [], [], []
        for p, s, tp, valid in self._batches:
            ps.append(p[valid].long())
            ss.append(s[valid])
            ts.append(tp[:, valid])
        return torch.cat(ps), torch.cat(ss), torch.cat(ts, 1)

    def merge(self, other):
        """Append another evaluator's records (its images after this one's) and add its accumulators."""
        if (other.ks, other.num_rel, other.topk, other.prd_k) != (self.ks, self.num_rel, self.topk, self.prd_k):
            raise ValueError("merge needs evaluators with the same ks, num_rel_labels, topk and prd_k")
        if other.acc is not None:
            self._acc_on(other.acc.device).add_(other.acc)
            self._batches += [tuple(x.to(self.acc.device) for x in b) for b in other._batches]
        return self

    def all_gather(self, group=None):
        """Gather the records of every rank of ``group`` (rank order, then update order) and sum the accumulators.
        No-op when torch.distributed is not initialised."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return self
        dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else \
            torch.device("cpu")
        if self.acc is None:
            self.acc = torch.zeros(self.width, dtype=torch.float64, device=dev)
        acc = self.acc.to(dev)
        dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=group)
        p, s, tp = (x.to(dev) for x in self._records())
        world = dist.get_world_size(group)
        n = torch.tensor([p.numel()], dtype=torch.int64, device=dev)
        sizes = [torch.zeros_like(n) for _ in range(world)]
        dist.all_gather(sizes, n, group=group)
        sizes = [int(x) for x in sizes]
        cap = max(sizes + [1])
        # one float64 buffer per rank: p, score (exact in float64), tp_rel, tp_phr
        buf = torch.zeros(4, cap, dtype=torch.float64, device=dev)
        buf[0, :p.numel()] = p.double()
        buf[1, :p.numel()] = s.double()
        buf[2:, :p.numel()] = tp.double()
        bufs = [torch.empty_like(buf) for _ in range(world)]
        dist.all_gather(bufs, buf, group=group)
        cat = torch.cat([b[:, :k] for b, k in zip(bufs, sizes)], 1)
        home = self.acc.device
        self.acc = acc.to(home)
        n_all = cat.shape[1]
        self._batches = [(cat[0].long()[None].to(home), cat[1].float()[None].to(home),
                          cat[2:].to(torch.uint8)[:, None].to(home), torch.ones(1, n_all, dtype=torch.bool, device=home))]
        return self

    # ---- update ----------------------------------------------------------------------------------------------------
    def update(self, candidates, targets):
        """Score one batch.  ``candidates``: ``runtime.triplet_candidates(mode="oi")`` output or dicts with pred_boxes,
        pred_classes, obj_scores, pred_scores [M, R] and sbj_obj_inds [M, 2] (optional on the device: absent = the
        row-major cartesian product); ``targets``: the reference's target dicts, on the host.  On the device path
        nothing is copied back and nothing waits."""
        if len(candidates) != len(targets):
            raise ValueError(f"{len(candidates)} candidate entries for {len(targets)} targets")
        if not candidates:
            return
        for c in candidates:
            for key in ("pred_boxes", "pred_classes", "obj_scores", "pred_scores"):
                if key not in c:
                    raise KeyError(f"candidate entry lacks {key!r}")
        shapes = {tuple(_tensor(c["pred_scores"]).shape) for c in candidates}
        if len(shapes) != 1:
            raise ValueError("every image of a batch needs the same pred_scores shape")
        shape = shapes.pop()
        if len(shape) != 2 or shape[1] != self.num_rel:
            raise ValueError(f"pred_scores must be [M, {self.num_rel}], got {shape}")
        if shape[0] > _OI_MAX_PAIRS:
            raise ValueError(f"at most {_OI_MAX_PAIRS} pairs per image, got {shape[0]}")
        if len({_tensor(c["pred_boxes"]).shape[0] for c in candidates}) != 1:
            raise ValueError("every image of a batch needs the same number of predicted boxes")
        for c in candidates:
            if "sbj_obj_inds" in c and tuple(_tensor(c["sbj_obj_inds"]).shape) != (shape[0], 2):
                raise ValueError(f"sbj_obj_inds must be [{shape[0]}, 2]")
        gts = [gt_entry(t) for t in targets]
        for g in gts:
            if g["gt_relations"].numel() and int(g["gt_relations"][:, 2].max()) >= self.num_rel:
                raise ValueError(f"a GT predicate is outside [0, {self.num_rel})")
            if g["gt_relations"].shape[0] > _OI_MAX_GT:
                raise ValueError(f"at most {_OI_MAX_GT} GT relations per image")
        ps = _tensor(candidates[0]["pred_scores"])
        if ps.device.type == "cpu":
            self._update_host(candidates, gts)
        else:
            self._update_device(candidates, gts, ps.device)

    def _row(self, fr, K, T, npos):
        """One slab row (float64 [W]) of an image, as oi_match writes it."""
        nk = len(self.ks)
        row = torch.zeros(self.width, dtype=torch.float64)
        if T == 0:
            row[2 * nk + 2] = 1.0
            return row
        hits = [int((fr < min(k, K)).sum()) for k in self.ks]
        row[:nk] = torch.tensor([float(h) / (float(T) + 1e-12) for h in hits], dtype=torch.float64)
        row[nk:2 * nk] = torch.tensor(hits, dtype=torch.float64)
        row[2 * nk] = float(T)
        row[2 * nk + 1] = 1.0
        row[2 * nk + 3:] = npos.double()
        return row

    def _update_host(self, candidates, gts):
        acc = self._acc_on(torch.device("cpu"))
        B, topk = len(candidates), self.topk
        p_out = torch.full((B, topk), -1, dtype=torch.int64)
        s_out = torch.zeros(B, topk, dtype=torch.float32)
        tp_out = torch.zeros(2, B, topk, dtype=torch.uint8)
        valid = torch.zeros(B, topk, dtype=torch.bool)
        rows, dets = [], []
        for b, (c, g) in enumerate(zip(candidates, gts)):
            ps = _tensor(c["pred_scores"]).float()
            boxes = _tensor(c["pred_boxes"]).float()
            classes = _tensor(c["pred_classes"]).long()
            N = boxes.shape[0]
            pairs = _tensor(c["sbj_obj_inds"]).long() if "sbj_obj_inds" in c else torch.cartesian_prod(
                torch.arange(N), torch.arange(N))
            if pairs.numel() and (int(pairs.min()) < 0 or int(pairs.max()) >= N):
                raise ValueError("sbj_obj_inds outside [0, num_boxes)")
            sop, score = oi_select_host(ps, _tensor(c["obj_scores"]).float(), pairs, topk, self.prd_k)
            dets.append((sop, score))
            T = g["gt_relations"].shape[0]
            K = sop.shape[0]
            fr = first_ranks_host(sop, boxes, classes, g["gt_relations"], g["gt_boxes"], g["gt_classes"], 0.5)
            npos = torch.bincount(g["gt_relations"][:, 2], minlength=self.num_rel) if T else \
                torch.zeros(self.num_rel, dtype=torch.int64)
            rows.append(self._row(fr, K, T, npos))
            if T:
                p_out[b, :K] = sop[:, 2]
                s_out[b, :K] = score
                tp_out[:, b, :K] = oi_tp_host(sop, boxes, classes, g["gt_relations"], g["gt_boxes"],
                                              g["gt_classes"]).to(torch.uint8)
                valid[b, :K] = True
        for r in rows:          # image order, like oi_fold
            acc.add_(r)
        self._batches.append((p_out, s_out, tp_out, valid))
        self.last_detections = dets
        self.last_rows = torch.stack(rows)

    _stage = SceneGraphRecall._stage   # the same pinned staging ring

    def _update_device(self, candidates, gts, device):
        acc = self._acc_on(device)
        B, topk, nk = len(candidates), self.topk, len(self.ks)
        ps = [c["pred_scores"] for c in candidates]
        M, R = ps[0].shape
        # the views triplet_candidates returns share one [B, N, N, R] tensor: pass its base and strides, no copy
        step = ps[1].data_ptr() - ps[0].data_ptr() if B > 1 else 0
        uniform = all(p.dtype == torch.float32 and p.device == device and p.stride(1) == 1 and
                      p.stride(0) == ps[0].stride(0) and p.stride(0) >= R for p in ps)
        uniform = uniform and all(p.untyped_storage().data_ptr() == ps[0].untyped_storage().data_ptr() and
                                  p.data_ptr() == ps[0].data_ptr() + b * step for b, p in enumerate(ps))
        uniform = uniform and (B == 1 or (step > 0 and step % 4 == 0))
        if uniform:
            scores, row_stride, img_stride = ps[0], ps[0].stride(0), step // 4
        else:
            scores = torch.stack([p.to(device, torch.float32) for p in ps]).contiguous()
            row_stride, img_stride = R, M * R
        obj = torch.stack([c["obj_scores"] for c in candidates]).to(torch.float32).contiguous()
        boxes = torch.stack([c["pred_boxes"] for c in candidates]).to(torch.float32).contiguous()
        classes = torch.stack([c["pred_classes"] for c in candidates]).to(torch.long).contiguous()
        N = boxes.shape[1]
        pl = [c.get("sbj_obj_inds") for c in candidates]
        if pl[0] is None:
            if any(x is not None for x in pl) or M != N * N:
                raise ValueError("without sbj_obj_inds every image needs the full N x N pair set")
            pairs, pair_stride = None, 0
        elif all(x is pl[0] for x in pl):
            pairs, pair_stride = pl[0].to(device, torch.long).contiguous(), 0
        else:
            pairs, pair_stride = torch.stack([x.to(device, torch.long) for x in pl]).contiguous(), M * 2
        h = _lib.lib()
        stream = torch.cuda.current_stream(device).cuda_stream
        ws = torch.empty(max(int(h.egtr_oi_select_workspace_bytes(M, topk, self.prd_k, B)), 8), dtype=torch.uint8,
                         device=device)
        sop = torch.empty(B, topk, 3, dtype=torch.int32, device=device)
        score = torch.empty(B, topk, dtype=torch.float32, device=device)
        count = torch.empty(B, dtype=torch.int32, device=device)
        _lib.check(h.egtr_oi_select_f32(stream, scores.data_ptr(), img_stride, row_stride, obj.data_ptr(),
                                        _lib.ptr(pairs), pair_stride, B, M, N, R, topk,
                                        self.prd_k, ws.data_ptr(), sop.data_ptr(), score.data_ptr(), count.data_ptr()),
                   "egtr_oi_select_f32")
        # ragged GT packed into one pinned buffer, as SceneGraphRecall:
        # int64 [rel_off B+1 | box_off B+1 | rels 3T | classes G], float32 boxes 4G
        rels = [g["gt_relations"] for g in gts]
        T = sum(r.shape[0] for r in rels)
        G = sum(g["gt_classes"].shape[0] for g in gts)
        n64 = 2 * (B + 1) + 3 * T + G
        nbytes = 8 * n64 + 16 * G
        buf, ev = self._stage(nbytes)
        i64 = buf[:8 * n64].view(torch.int64)
        f32 = buf[8 * n64:nbytes].view(torch.float32)
        i64[:B + 1] = torch.tensor([0] + [r.shape[0] for r in rels], dtype=torch.int64).cumsum(0)
        i64[B + 1:2 * B + 2] = torch.tensor([0] + [g["gt_classes"].shape[0] for g in gts], dtype=torch.int64).cumsum(0)
        if T:
            i64[2 * B + 2:2 * B + 2 + 3 * T] = torch.cat(rels).reshape(-1)
        if G:
            i64[2 * B + 2 + 3 * T:] = torch.cat([g["gt_classes"] for g in gts])
            f32.copy_(torch.cat([g["gt_boxes"] for g in gts]).reshape(-1))
        dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        dev.copy_(buf[:nbytes], non_blocking=True)
        ev.record()
        d64 = dev[:8 * n64].view(torch.int64)
        d_boxes = dev[8 * n64:].view(torch.float32)
        slab = torch.empty(B, self.width, dtype=torch.float64, device=device)
        tp = torch.empty(2, B, topk, dtype=torch.uint8, device=device)
        ks = (ctypes.c_int * nk)(*self.ks)
        _lib.check(h.egtr_oi_match_f32(
            stream, sop.data_ptr(), count.data_ptr(), B, topk, boxes.data_ptr(), classes.data_ptr(), N, self.num_rel,
            d64[2 * B + 2:].data_ptr() if T else None, d64.data_ptr(), T, d_boxes.data_ptr() if G else None,
            d64[2 * B + 2 + 3 * T:].data_ptr() if G else None, d64[B + 1:].data_ptr(), G, ks, nk, tp.data_ptr(),
            slab.data_ptr(), acc.data_ptr()), "egtr_oi_match_f32")
        valid = (torch.arange(topk, device=device)[None, :] < count[:, None]) & (slab[:, 2 * nk + 2:2 * nk + 3] == 0)
        self._batches.append((sop[:, :, 2], score, tp, valid))
        self.last_detections = (sop, score, count)
        self.last_rows = slab

    # ---- results (one synchronisation) -------------------------------------------------------------------------------
    def _ap(self):
        """AP [2, C] (rel, phr) as float64 on the host, and npos [C] (ints)."""
        C = self.num_rel
        nk = len(self.ks)
        a = self.acc if self.acc is not None else torch.zeros(self.width, dtype=torch.float64)
        npos_t = a[2 * nk + 3:].contiguous()
        p, s, tp = self._records()
        key = (p << 32) | (0xFFFFFFFF - (s.view(torch.int32).long() & 0xFFFFFFFF))
        perm = torch.sort(key, stable=True).indices
        seg = torch.zeros(C + 1, dtype=torch.int64, device=p.device)
        seg[1:] = torch.cumsum(torch.bincount(p, minlength=C)[:C], 0)
        tps = tp[:, perm].contiguous()
        n = int(p.numel())
        if p.device.type == "cpu":
            npos = [int(v) for v in npos_t.tolist()]
            segs = seg.tolist()
            ap = torch.tensor([[oi_ap_host(tps[m, segs[c]:segs[c + 1]].bool(), segs[c + 1] - segs[c], npos[c])
                                for c in range(C)] for m in range(2)], dtype=torch.float64)
            return ap, npos
        out = torch.empty(2, C, dtype=torch.float64, device=p.device)
        scratch = torch.empty(max(4 * n, 1), dtype=torch.float64, device=p.device)
        stream = torch.cuda.current_stream(p.device).cuda_stream
        _lib.check(_lib.lib().egtr_oi_ap_f64(stream, tps.data_ptr(), seg.data_ptr(), npos_t.data_ptr(), n, C,
                                             scratch.data_ptr(), out.data_ptr()), "egtr_oi_ap_f64")
        return out.cpu(), [int(v) for v in npos_t.tolist()]

    def _host_acc(self):
        if self.acc is None:
            return torch.zeros(self.width, dtype=torch.float64)
        return self.acc.cpu()

    def per_class(self):
        """{c: {"rel_AP", "phr_AP", "w_rel_AP", "w_phr_AP", "npos"}} for every predicate class (eval_rel_results'
        per-class lines: weighted AP = AP * npos_c / sum npos)."""
        ap, npos = self._ap()
        all_npos = sum(npos)
        out = {}
        for c in range(self.num_rel):
            r, ph = float(ap[0, c]), float(ap[1, c])
            out[c] = {"rel_AP": r, "phr_AP": ph, "npos": npos[c],
                      "w_rel_AP": r * float(npos[c]) / float(all_npos) if all_npos else float("nan"),
                      "w_phr_AP": ph * float(npos[c]) / float(all_npos) if all_npos else float("nan")}
        return out

    def compute(self):
        """The reference's keys (w_rel_mAP, w_phr_mAP, microR@50, score) plus rel_mAP, phr_mAP, microR@k and the
        per-image mean R@k for every k.  Sums run in class order like eval_rel_results."""
        a = self._host_acc().tolist()
        nk = len(self.ks)
        ap, npos = self._ap()
        all_npos = sum(npos)
        out = {}
        for mode, name in enumerate(("rel", "phr")):
            s = w = 0.0
            for c in range(self.num_rel):
                v = float(ap[mode, c])
                w += v * float(npos[c]) / float(all_npos) if all_npos else float("nan")
                s += v
            out[f"{name}_mAP"] = s / self.num_rel
            out[f"w_{name}_mAP"] = w
        n_img, n_gt = a[2 * nk + 1], a[2 * nk]
        for j, k in enumerate(self.ks):
            out[f"microR@{k}"] = a[nk + j] / (n_gt + 1e-12)
            out[f"R@{k}"] = a[j] / n_img if n_img > 0 else float("nan")
        if 50 in self.ks:
            out["score"] = out["w_rel_mAP"] * 0.4 + out["w_phr_mAP"] * 0.4 + out["microR@50"] * 0.2
        return out

    @property
    def n_images(self):
        return int(self._host_acc()[2 * len(self.ks) + 1])

    @property
    def skipped(self):
        return int(self._host_acc()[2 * len(self.ks) + 2])


# ---- COCO box detection metrics -----------------------------------------------------------------------------------------
# pycocotools Params(iouType="bbox"), built with numpy exactly as Params.setDetParams builds them
COCO_IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
COCO_REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
COCO_MAX_DETS = (1, 10, 100)
COCO_AREA_RNGS = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))
COCO_STATS = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")
_COCO_MAX_DET, _COCO_MAX_GT, _COCO_MAX_CLS = 1024, 1024, 1024
_EPS = float(np.spacing(1))


def coco_gt_entry(target):
    """The COCO GT of one of the reference's target dicts, on the host: boxes fp64 xywh from ``rescale_bboxes`` (w = x1 -
    x0 in fp64 on the fp32 corners), area = target area * orig_h * orig_w / (size_h * size_w) when the target carries
    ``area`` and ``size`` (the resize scaled it), else the box w * h; iscrowd if present, else 0.  Reconstructed boxes
    and areas can differ from the dataset's COCO json by float rounding; pass explicit GT dicts for exact parity."""
    t = {k: (v.cpu() if torch.is_tensor(v) else torch.as_tensor(v)) for k, v in target.items()}
    xyxy = rescale_bboxes(t["boxes"].float().reshape(-1, 4), t["orig_size"]).double()
    boxes = torch.cat([xyxy[:, :2], xyxy[:, 2:] - xyxy[:, :2]], 1)
    if "area" in t and "size" in t:
        oh, ow = float(t["orig_size"][0]), float(t["orig_size"][1])
        sh, sw = float(t["size"][0]), float(t["size"][1])
        area = t["area"].double().reshape(-1) * (oh * ow) / (sh * sw)
    else:
        area = boxes[:, 2] * boxes[:, 3]
    n = boxes.shape[0]
    crowd = t["iscrowd"].reshape(-1).to(torch.uint8) if "iscrowd" in t else torch.zeros(n, dtype=torch.uint8)
    return {"boxes": boxes, "area": area, "iscrowd": crowd, "labels": t["class_labels"].long().reshape(-1)}


def _coco_gt(g):
    """Normalise one GT argument of CocoDetectionMetrics.update (a target dict or an explicit COCO GT dict)."""
    if "class_labels" in g:
        return coco_gt_entry(g)
    for key in ("boxes", "labels"):
        if key not in g:
            raise KeyError(f"GT entry lacks {key!r}")
    boxes = _tensor(g["boxes"]).cpu().double().reshape(-1, 4)
    n = boxes.shape[0]
    area = _tensor(g["area"]).cpu().double().reshape(-1) if "area" in g else boxes[:, 2] * boxes[:, 3]
    crowd = _tensor(g["iscrowd"]).cpu().reshape(-1).to(torch.uint8) if "iscrowd" in g else \
        torch.zeros(n, dtype=torch.uint8)
    labels = _tensor(g["labels"]).cpu().long().reshape(-1)
    if area.shape[0] != n or crowd.shape[0] != n or labels.shape[0] != n:
        raise ValueError("GT boxes, area, iscrowd and labels need the same length")
    return {"boxes": boxes, "area": area, "iscrowd": crowd, "labels": labels}


def _score_key(s):
    """Order key of float32 scores as int64 in [0, 2^32): larger key = higher score, -0 == +0 (the kernels' score_key)."""
    u = s.contiguous().view(torch.int32).long() & 0xFFFFFFFF
    u = torch.where(u == 0x80000000, torch.zeros_like(u), u)
    return torch.where(u >= 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def _segment_rank(group):
    """Position of every element within its run of equal values of the sorted int64 ``group``."""
    n = group.numel()
    idx = torch.arange(n, device=group.device)
    if n == 0:
        return idx
    start = torch.ones(n, dtype=torch.bool, device=group.device)
    start[1:] = group[1:] != group[:-1]
    return idx - torch.where(start, idx, 0).cummax(0).values


def coco_iou_host(d, g, crowd):
    """maskApi bbIou between broadcast rows of d [..., 4] and g [..., 4] (fp64 xywh): ``crowd`` (bool, broadcast like the
    rows) makes the union the detection's area.  The C loop's operation order."""
    dx, dy, dw, dh = d.unbind(-1)
    gx, gy, gw, gh = g.unbind(-1)
    da, ga = dw * dh, gw * gh
    w = torch.minimum(dw + dx, gw + gx) - torch.maximum(dx, gx)
    h = torch.minimum(dh + dy, gh + gy) - torch.maximum(dy, gy)
    i = w * h
    u = torch.where(crowd, da, da + ga - i)
    return torch.where((w > 0) & (h > 0), i / u, torch.zeros((), dtype=torch.float64))


def coco_match_host(scores, labels, boxes, gts, num_classes, max_det=COCO_MAX_DETS[-1]):
    """evaluateImg of every (image, category) of one batch on the host, vectorised over the (image, category) pairs, the
    thresholds, the area ranges and the GTs; a loop over the in-category rank.  scores [B, D] fp32, labels [B, D] int64,
    boxes [B, D, 4] fp32 xyxy; gts: per image {"boxes" fp64 xywh, "area", "iscrowd", "labels"}.
    Returns (label int32 [B, D] (-1 = no record), rank int32 [B, D] (-1 = no record), bits int64 [B, D, 2] (match,
    ignore; bit t * A + a), npig int32 [K, A]) -- what egtr_coco_match_f32 writes."""
    K, T, A = num_classes, len(COCO_IOU_THRS), len(COCO_AREA_RNGS)
    B, D = labels.shape
    n = B * D
    lab = labels.reshape(-1).long()
    valid = (lab >= 0) & (lab < K)
    key = _score_key(scores.reshape(-1).float())
    # rank within (image, category): descending score, ties to the lower index
    group = torch.where(valid, torch.arange(n) // D * (K + 1) + lab, torch.arange(n) // D * (K + 1) + K)
    o1 = torch.sort(-key, stable=True).indices
    o2 = o1[torch.sort(group[o1], stable=True).indices]
    rank = torch.empty(n, dtype=torch.long)
    rank[o2] = _segment_rank(group[o2])
    rank = torch.where(valid & (rank < max_det), rank, -1)
    rec_label = torch.where(rank >= 0, lab, -1)
    bits = torch.zeros(n, 2, dtype=torch.int64)

    lo = torch.tensor([r[0] for r in COCO_AREA_RNGS], dtype=torch.float64)
    hi = torch.tensor([r[1] for r in COCO_AREA_RNGS], dtype=torch.float64)
    g_img = torch.cat([torch.full((g["labels"].shape[0],), b, dtype=torch.long) for b, g in enumerate(gts)]) \
        if gts else torch.zeros(0, dtype=torch.long)
    g_lab = torch.cat([g["labels"] for g in gts]) if gts else torch.zeros(0, dtype=torch.long)
    g_box = torch.cat([g["boxes"] for g in gts]).reshape(-1, 4) if gts else torch.zeros(0, 4, dtype=torch.float64)
    g_area = torch.cat([g["area"] for g in gts]) if gts else torch.zeros(0, dtype=torch.float64)
    g_crowd = torch.cat([g["iscrowd"] for g in gts]).bool() if gts else torch.zeros(0, dtype=torch.bool)
    g_ig = g_crowd[None] | (g_area[None] < lo[:, None]) | (g_area[None] > hi[:, None])            # [A, NG]
    npig = torch.zeros(K * A, dtype=torch.int64)
    gv = (g_lab >= 0) & (g_lab < K)
    if bool(gv.any()):
        idx = (g_lab[gv][None] * A + torch.arange(A)[:, None]).reshape(-1)
        npig.index_add_(0, idx, (~g_ig[:, gv]).reshape(-1).long())
    npig = npig.reshape(K, A).to(torch.int32)

    kept = torch.nonzero(rank >= 0).flatten()
    gsel = torch.nonzero(gv).flatten()
    if kept.numel() == 0:
        return rec_label.reshape(B, D).int(), rank.reshape(B, D).int(), bits.reshape(B, D, 2), npig
    # (image, category) pairs with a kept detection; pairs with GT only change nothing but npig
    d_pair = (kept // D) * K + lab[kept]
    g_pair = g_img[gsel] * K + g_lab[gsel]
    pairs, inv = torch.unique(d_pair, return_inverse=True)
    P = pairs.numel()
    Dm = int(rank[kept].max()) + 1
    dtab = torch.full((P, Dm), -1, dtype=torch.long)
    dtab[inv, rank[kept]] = kept
    g_in = torch.isin(g_pair, pairs)
    gsel, g_pair = gsel[g_in], g_pair[g_in]
    go = torch.sort(g_pair, stable=True).indices
    gsel, g_pair = gsel[go], g_pair[go]
    g_pos = _segment_rank(g_pair)
    g_p = torch.searchsorted(pairs, g_pair)
    Gm = int(g_pos.max()) + 1 if gsel.numel() else 1
    gtab = torch.full((P, Gm), -1, dtype=torch.long)
    if gsel.numel():
        gtab[g_p, g_pos] = gsel
    gex = gtab >= 0
    gi = gtab.clamp(min=0)
    gb = torch.where(gex[..., None], g_box[gi] if g_box.shape[0] else torch.zeros(P, Gm, 4, dtype=torch.float64), 0.0)
    crowd = gex & (g_crowd[gi] if g_crowd.numel() else torch.zeros(P, Gm, dtype=torch.bool))
    ig = gex[None] & (g_ig[:, gi] if g_ig.shape[1] else torch.zeros(A, P, Gm, dtype=torch.bool))       # [A, P, Gm]
    xyxy = boxes.reshape(-1, 4).float()
    wh = xyxy[:, 2:] - xyxy[:, :2]                                                          # fp32, like convert_to_xywh
    dxywh = torch.cat([xyxy[:, :2].double(), wh.double()], 1)
    d_area = dxywh[:, 2] * dxywh[:, 3]

    thr = torch.tensor([min(float(t), 1 - 1e-10) for t in COCO_IOU_THRS], dtype=torch.float64)[:, None, None, None]
    shift = (torch.arange(T)[:, None] * A + torch.arange(A)[None, :])[:, :, None]           # [T, A, 1]
    gidx = torch.arange(Gm)
    matched = torch.zeros(T, A, P, Gm, dtype=torch.bool)

    def last_max(cand, iou):
        v = torch.where(cand, iou, float("-inf"))
        mx = v.max(-1, keepdim=True).values
        return torch.where(cand & (v == mx), gidx, -1).max(-1).values

    for r in range(Dm):
        d = dtab[:, r]
        has = d >= 0
        dd = d.clamp(min=0)
        iou = coco_iou_host(dxywh[dd][:, None, :], gb, crowd)                               # [P, Gm]
        iou = torch.where(gex, iou, 0.0)[None, None]
        hit = iou >= thr                                                                     # [T, 1, P, Gm]
        m1 = last_max(gex & ~ig & ~matched & hit, iou)
        m2 = last_max(gex & ig & (~matched | crowd) & hit, iou)
        m = torch.where(m1 >= 0, m1, m2)
        m = torch.where(has, m, -1)                                                          # [T, A, P]
        found = m >= 0
        matched |= gidx == m[..., None]
        mig = torch.gather(ig[None].expand(T, A, P, Gm), 3, m.clamp(min=0)[..., None])[..., 0] & found
        out = (d_area[dd][None] < lo[:, None]) | (d_area[dd][None] > hi[:, None])           # [A, P]
        dig = torch.where(found, mig, out[None])
        mb = (found.long() << shift).sum((0, 1))
        ib = ((dig & has).long() << shift).sum((0, 1))
        bits[d[has], 0] = mb[has]
        bits[d[has], 1] = ib[has]
    return rec_label.reshape(B, D).int(), rank.reshape(B, D).int(), bits.reshape(B, D, 2), npig


def coco_accumulate_host(rank_s, bits_s, seg, npig, num_classes):
    """accumulate over records sorted by (category, score descending, image, rank), on the host: precision
    [T, R, K, A, M] and recall [T, K, A, M] in fp64 -- the same terms as the coco_accumulate kernel."""
    K, T, A, M, R = num_classes, len(COCO_IOU_THRS), len(COCO_AREA_RNGS), len(COCO_MAX_DETS), len(COCO_REC_THRS)
    n = int(seg[K])
    precision = torch.full((T, R, K, A, M), -1.0, dtype=torch.float64)
    recall = torch.full((T, K, A, M), -1.0, dtype=torch.float64)
    rank_s, bits_s = rank_s[:n].long(), bits_s[:n]
    cat = torch.repeat_interleave(torch.arange(K), seg[1:] - seg[:-1])
    shift = torch.arange(T)[:, None] * A + torch.arange(A)[None, :]
    rthr = torch.from_numpy(COCO_REC_THRS.astype(np.float64))
    npd = npig.double()
    have = npig > 0                                                                          # [K, A]
    for mi, md in enumerate(COCO_MAX_DETS):
        ki = torch.nonzero((rank_s >= 0) & (rank_s < md)).flatten()
        lab = cat[ki]
        nk = torch.zeros(K, dtype=torch.long).index_add_(0, lab, torch.ones_like(lab))
        end = torch.cumsum(nk, 0)
        start = end - nk
        for a in range(A):                   # one area range at a time keeps the [n, T] temporaries small
            mb = (bits_s[ki, 0][:, None] >> shift[:, a]) & 1
            ib = (bits_s[ki, 1][:, None] >> shift[:, a]) & 1
            zero = torch.zeros(1, T, dtype=torch.long)
            ctp0 = torch.cat([zero, torch.cumsum(mb & (1 - ib), 0)])
            cfp0 = torch.cat([zero, torch.cumsum((1 - mb) & (1 - ib), 0)])
            tpd = (ctp0[1:] - ctp0[start][lab]).double()
            fpd = (cfp0[1:] - cfp0[start][lab]).double()
            rc = tpd / npd[lab, a][:, None]
            pr = tpd / ((fpd + tpd) + _EPS)
            bucket = torch.searchsorted(rthr, rc.reshape(-1).contiguous(), right=True).reshape(rc.shape) - 1
            flat = (lab[:, None] * T + torch.arange(T)[None, :]) * R + bucket
            q = torch.zeros(K * T * R, dtype=torch.float64).scatter_reduce_(0, flat.reshape(-1), pr.reshape(-1), "amax")
            q = q.reshape(K, T, R).flip(-1).cummax(-1).values.flip(-1)
            last = (ctp0[end] - ctp0[start]).double() / npd[:, a][:, None]                 # [K, T]
            rec = torch.where((nk > 0)[:, None], last, 0.0)
            ok = have[:, a]
            precision[:, :, :, a, mi] = torch.where(ok[None, None], q.permute(1, 2, 0), -1.0)
            recall[:, :, a, mi] = torch.where(ok[None], rec.t(), -1.0)
    return precision, recall


def coco_summarize(precision, recall):
    """summarize's 12 stats as an fp64 tensor on the tensors' device (mean of the entries > -1, -1 if none)."""
    t50 = int(np.where(0.5 == COCO_IOU_THRS)[0][0])
    t75 = int(np.where(0.75 == COCO_IOU_THRS)[0][0])
    m100 = COCO_MAX_DETS.index(100)

    def mean(s):
        ok = s > -1
        cnt = ok.sum()
        return torch.where(cnt > 0, torch.where(ok, s, 0.0).sum() / cnt.clamp(min=1), -1.0)

    p, r = precision, recall
    return torch.stack([mean(p[:, :, :, 0, m100]), mean(p[t50, :, :, 0, m100]), mean(p[t75, :, :, 0, m100]),
                        mean(p[:, :, :, 1, m100]), mean(p[:, :, :, 2, m100]), mean(p[:, :, :, 3, m100]),
                        mean(r[:, :, 0, 0]), mean(r[:, :, 0, 1]), mean(r[:, :, 0, m100]),
                        mean(r[:, :, 1, m100]), mean(r[:, :, 2, m100]), mean(r[:, :, 3, m100])])


class CocoDetectionMetrics:
    """COCO box-detection AP / AR of pycocotools ``COCOeval(iouType="bbox")`` as the reference's ``CocoEvaluator`` runs
    it (evaluate + accumulate + summarize; lib/evaluation/coco_eval.py): iouThrs .50:.05:.95, 101 recall thresholds,
    maxDets (1, 10, 100), area ranges all / small / medium / large (bounds inclusive), categories 0 .. num_classes-1.

    ``update(results, gts)``: ``results`` is ``DeformableDetrFeatureExtractor.post_process`` output (scores, labels,
    boxes as absolute fp32 xyxy per image); a label outside [0, num_classes) is not evaluated.  ``gts`` per image: the
    reference's target dicts (through ``coco_gt_entry``) or explicit dicts {"boxes" fp64 xywh, "area", "iscrowd",
    "labels"} -- exact parity with a COCO json needs the explicit form.  Device tensors go to egtr_coco_match_f32
    (csrc/coco_eval.hip) without a host synchronisation; host tensors to ``coco_match_host``.  Every detection leaves a
    record (label, score, in-category rank, match and ignore bits per (threshold, area range)); npig [K, A] counts the
    non-ignored GTs.  ``compute`` sorts the records by (category, score descending, image, rank) once, runs
    accumulate (egtr_coco_accumulate_f64 or ``coco_accumulate_host``) and returns the 12 stats with one synchronisation.

    Stated differences and limits:
      * image order is the order of ``update`` calls; CocoEvaluator sorts by image id, so the two agree whenever ids rise
        with update order -- it only matters for equal scores across images;
      * a match is a flag, not a GT id: pycocotools takes a match to a GT whose annotation id is 0 for no match (the OI
        detection path numbers its GT ids from 0, the VG path does not);
      * OICocoEvaluator (+1 widths) is not built in; a caller who builds its boxes, areas and labels gets its numbers;
      * NaN scores or boxes are not supported; at most 1024 detections and 1024 GTs per image and 1024 categories on
        the device (ValueError); the host path has no caps."""

    def __init__(self, num_classes):
        if not 1 <= num_classes <= _COCO_MAX_CLS:
            raise ValueError(f"num_classes must be in [1, {_COCO_MAX_CLS}], got {num_classes}")
        self.num_classes = int(num_classes)
        self._ring = []            # [pinned buffer, event] staging slots of the host -> device GT copies
        self.reset()

    _stage = SceneGraphRecall._stage   # the same pinned staging ring

    # ---- state -----------------------------------------------------------------------------------------------------
    def reset(self):
        self.npig = None           # int32 [K, A] on the device of the first update
        self._batches = []         # (label int32 [B, D], score fp32 [B, D], rank int32 [B, D], bits int64 [B, D, 2])
        self._n_images = 0
        self._result = None
        self.last_matches = None

    def _npig_on(self, device):
        if self.npig is None:
            self.npig = torch.zeros(self.num_classes, len(COCO_AREA_RNGS), dtype=torch.int32, device=device)
        elif self.npig.device != device:
            raise ValueError(f"this evaluator accumulates on {self.npig.device}, got inputs on {device}")
        return self.npig

    @property
    def n_images(self):
        return self._n_images

    def merge(self, other):
        """Append another evaluator's records (its images after this one's) and add its GT counts."""
        if other.num_classes != self.num_classes:
            raise ValueError("merge needs evaluators with the same num_classes")
        if other.npig is not None:
            dev = self._npig_on(other.npig.device if self.npig is None else self.npig.device).device
            self.npig.add_(other.npig.to(dev))
            self._batches += [tuple(x.to(dev) for x in b) for b in other._batches]
        self._n_images += other._n_images
        self._result = None
        return self

    def all_gather(self, group=None):
        """Gather the records of every rank of ``group`` (rank order, then update order) and sum the GT counts and image
        counts.  No-op when torch.distributed is not initialised."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return self
        dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else \
            torch.device("cpu")
        K, A = self.num_classes, len(COCO_AREA_RNGS)
        home = self.npig.device if self.npig is not None else dev
        acc = torch.zeros(K * A + 1, dtype=torch.int64, device=dev)
        if self.npig is not None:
            acc[:K * A] = self.npig.reshape(-1).to(dev).long()
        acc[K * A] = self._n_images
        dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=group)
        label, score, rank, bits = (x.to(dev) for x in self._records())
        world = dist.get_world_size(group)
        n = torch.tensor([label.numel()], dtype=torch.int64, device=dev)
        sizes = [torch.zeros_like(n) for _ in range(world)]
        dist.all_gather(sizes, n, group=group)
        sizes = [int(x) for x in sizes]
        cap = max(sizes + [1])
        buf = torch.zeros(5, cap, dtype=torch.int64, device=dev)   # label, score bits, rank, match bits, ignore bits
        k = label.numel()
        buf[0, :k] = label.long()
        buf[1, :k] = score.contiguous().view(torch.int32).long()
        buf[2, :k] = rank.long()
        buf[3:, :k] = bits.t()
        bufs = [torch.empty_like(buf) for _ in range(world)]
        dist.all_gather(bufs, buf, group=group)
        cat = torch.cat([b[:, :s] for b, s in zip(bufs, sizes)], 1)
        self.npig = acc[:K * A].reshape(K, A).to(torch.int32).to(home)
        self._n_images = int(acc[K * A])
        self._batches = [(cat[0].int()[None].to(home), cat[1].int().view(torch.float32)[None].to(home),
                          cat[2].int()[None].to(home), cat[3:].t().contiguous()[None].to(home))]
        self._result = None
        return self

    def _records(self):
        """Flat records in image order: (label int32 [n], score fp32 [n], rank int32 [n], bits int64 [n, 2])."""
        dev = self.npig.device if self.npig is not None else torch.device("cpu")
        if not self._batches:
            return (torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.float32, device=dev),
                    torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, 2, dtype=torch.int64, device=dev))
        return (torch.cat([b[0].reshape(-1) for b in self._batches]), torch.cat([b[1].reshape(-1) for b in self._batches]),
                torch.cat([b[2].reshape(-1) for b in self._batches]),
                torch.cat([b[3].reshape(-1, 2) for b in self._batches]))

    # ---- update ----------------------------------------------------------------------------------------------------
    def update(self, results, gts):
        """Score one batch: ``results`` (post_process output) and ``gts`` (target dicts or explicit GT dicts), one per
        image.  On the device path nothing is copied back and nothing waits."""
        if len(results) != len(gts):
            raise ValueError(f"{len(results)} result entries for {len(gts)} GT entries")
        if not results:
            return
        for r in results:
            for key in ("scores", "labels", "boxes"):
                if key not in r:
                    raise KeyError(f"result entry lacks {key!r}")
            n = _tensor(r["scores"]).shape[0]
            if tuple(_tensor(r["labels"]).shape) != (n,) or tuple(_tensor(r["boxes"]).shape) != (n, 4):
                raise ValueError("a result needs scores [D], labels [D] and boxes [D, 4]")
        g = [_coco_gt(x) for x in gts]
        for x in g:
            if x["labels"].numel() and (int(x["labels"].min()) < 0 or int(x["labels"].max()) >= self.num_classes):
                raise ValueError(f"a GT label is outside [0, {self.num_classes})")
        device = _tensor(results[0]["scores"]).device
        scores, labels, boxes = self._stack(results, device)
        self._result = None
        if device.type == "cpu":
            npig = self._npig_on(device)
            label, rank, bits, n = coco_match_host(scores, labels, boxes, g, self.num_classes)
            npig.add_(n)
        else:
            label, rank, bits = self._update_device(scores, labels, boxes, g, device)
        self._batches.append((label, scores.float().contiguous(), rank, bits))
        self._n_images += len(results)
        self.last_matches = {"label": label, "rank": rank, "match": bits[..., 0], "ignore": bits[..., 1]}

    @staticmethod
    def _stack(results, device):
        def stacked(key, dtype, pad):
            ts = [_tensor(r[key]).to(device, dtype) for r in results]
            if len(ts) == 1:
                return ts[0].unsqueeze(0).contiguous()
            if len({t.shape[0] for t in ts}) == 1:
                return torch.stack(ts).contiguous()
            return torch.nn.utils.rnn.pad_sequence(ts, batch_first=True, padding_value=pad).contiguous()
        return (stacked("scores", torch.float32, 0.0), stacked("labels", torch.long, -1),
                stacked("boxes", torch.float32, 0.0))

    def _update_device(self, scores, labels, boxes, g, device):
        B, D = labels.shape
        if D > _COCO_MAX_DET:
            raise ValueError(f"at most {_COCO_MAX_DET} detections per image on the device, got {D}")
        counts = [x["labels"].shape[0] for x in g]
        if max(counts) > _COCO_MAX_GT:
            raise ValueError(f"at most {_COCO_MAX_GT} GTs per image on the device, got {max(counts)}")
        npig = self._npig_on(device)
        G = sum(counts)
        # ragged GT packed into one pinned buffer: int64 [offsets B+1 | labels G], fp64 [boxes 4G | area G], u8 crowd G
        n64 = B + 1 + G
        nbytes = 8 * n64 + 40 * G + G
        buf, ev = self._stage(nbytes)
        i64 = buf[:8 * n64].view(torch.int64)
        f64 = buf[8 * n64:8 * n64 + 40 * G].view(torch.float64)
        i64[:B + 1] = torch.tensor([0] + counts, dtype=torch.int64).cumsum(0)
        if G:
            i64[B + 1:] = torch.cat([x["labels"] for x in g])
            f64[:4 * G] = torch.cat([x["boxes"] for x in g]).reshape(-1)
            f64[4 * G:] = torch.cat([x["area"] for x in g])
            buf[8 * n64 + 40 * G:nbytes] = torch.cat([x["iscrowd"] for x in g])
        dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        dev.copy_(buf[:nbytes], non_blocking=True)
        ev.record()
        d64 = dev[:8 * n64].view(torch.int64)
        df = dev[8 * n64:8 * n64 + 40 * G].view(torch.float64)
        label = torch.empty(B, D, dtype=torch.int32, device=device)
        score = torch.empty(B, D, dtype=torch.float32, device=device)
        rank = torch.empty(B, D, dtype=torch.int32, device=device)
        bits = torch.empty(B, D, 2, dtype=torch.int64, device=device)
        thr = (ctypes.c_double * len(COCO_IOU_THRS))(*[float(t) for t in COCO_IOU_THRS])
        rng = (ctypes.c_double * (2 * len(COCO_AREA_RNGS)))(*[float(v) for r in COCO_AREA_RNGS for v in r])
        stream = torch.cuda.current_stream(device).cuda_stream
        _lib.check(_lib.lib().egtr_coco_match_f32(
            stream, boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), B, D, self.num_classes,
            df[:4 * G].data_ptr() if G else None, df[4 * G:].data_ptr() if G else None,
            dev[8 * n64 + 40 * G:].data_ptr() if G else None, d64[B + 1:].data_ptr() if G else None, d64.data_ptr(), G,
            thr, rng, COCO_MAX_DETS[-1], label.data_ptr(), score.data_ptr(), rank.data_ptr(), bits.data_ptr(),
            npig.data_ptr()), "egtr_coco_match_f32")
        return label, rank, bits

    # ---- results (one synchronisation) -------------------------------------------------------------------------------
    def _accumulate(self):
        """(precision [T, R, K, A, M], recall [T, K, A, M]) fp64 on the records' device, cached until the next update."""
        if self._result is not None:
            return self._result
        K = self.num_classes
        label, score, rank, bits = self._records()
        dev = label.device
        npig = self.npig if self.npig is not None else \
            torch.zeros(K, len(COCO_AREA_RNGS), dtype=torch.int32, device=dev)
        p = torch.where(rank >= 0, label.long(), K)
        key = (p << 32) | (0xFFFFFFFF - _score_key(score))
        perm = torch.sort(key, stable=True).indices
        rank_s, bits_s = rank[perm].contiguous(), bits[perm].contiguous()
        seg = torch.zeros(K + 1, dtype=torch.int64, device=dev)
        seg[1:] = torch.cumsum(torch.zeros(K + 1, dtype=torch.int64, device=dev).scatter_add_(
            0, p, torch.ones_like(p))[:K], 0)
        if dev.type == "cpu":
            self._result = coco_accumulate_host(rank_s, bits_s, seg, npig, K)
            return self._result
        T, A, M, R = len(COCO_IOU_THRS), len(COCO_AREA_RNGS), len(COCO_MAX_DETS), len(COCO_REC_THRS)
        precision = torch.empty(T, R, K, A, M, dtype=torch.float64, device=dev)
        recall = torch.empty(T, K, A, M, dtype=torch.float64, device=dev)
        md = (ctypes.c_int * M)(*COCO_MAX_DETS)
        rt = (ctypes.c_double * R)(*[float(v) for v in COCO_REC_THRS])
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.lib().egtr_coco_accumulate_f64(
            stream, rank_s.data_ptr(), bits_s.data_ptr(), seg.data_ptr(), npig.contiguous().data_ptr(), rank_s.numel(),
            K, md, rt, precision.data_ptr(), recall.data_ptr()), "egtr_coco_accumulate_f64")
        self._result = (precision, recall)
        return self._result

    @property
    def precision(self):
        """accumulate's precision [T, R, K, A, M] (fp64, -1 where a category has no non-ignored GT)."""
        return self._accumulate()[0]

    @property
    def recall(self):
        """accumulate's recall [T, K, A, M] (fp64, -1 where a category has no non-ignored GT)."""
        return self._accumulate()[1]

    def compute(self):
        """summarize's 12 stats: {"AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm",
        "ARl"}."""
        precision, recall = self._accumulate()
        return dict(zip(COCO_STATS, coco_summarize(precision, recall).tolist()))

    def per_class(self):
        """{k: {"AP", "AP50", "AP75", "AR100"}} over area "all" and maxDets 100 for every category (-1 where the
        category has no non-ignored GT)."""
        precision, recall = self._accumulate()
        t50 = int(np.where(0.5 == COCO_IOU_THRS)[0][0])
        t75 = int(np.where(0.75 == COCO_IOU_THRS)[0][0])
        m = COCO_MAX_DETS.index(100)
        p = precision[:, :, :, 0, m]                                                         # [T, R, K]
        r = recall[:, :, 0, m]                                                               # [T, K]

        def mean(s, dims):
            ok = s > -1
            cnt = ok.sum(dims)
            return torch.where(cnt > 0, torch.where(ok, s, 0.0).sum(dims) / cnt.clamp(min=1), -1.0)

        rows = torch.stack([mean(p, (0, 1)), mean(p[t50], (0,)), mean(p[t75], (0,)), mean(r, (0,))], 1).cpu().tolist()
        return {k: dict(zip(("AP", "AP50", "AP75", "AR100"), row)) for k, row in enumerate(rows)}
