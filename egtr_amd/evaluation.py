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
relations is skipped and counted (the reference raises a KeyError).  The COCO detection metrics are not computed.
"""
import ctypes
import math

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
            stream, inds.data_ptr(), inds.shape[2], scores.data_ptr() if scores is not None else None, boxes.data_ptr(),
            classes.data_ptr(), B, K, N, self.num_rel, d64[2 * B + 2:].data_ptr() if T else None, d64.data_ptr(), T,
            d_boxes.data_ptr() if G else None, d64[2 * B + 2 + 3 * T:].data_ptr() if G else None,
            d64[B + 1:].data_ptr(), G, ks, len(self.ks), self.iou_thresh, first_rank.data_ptr(), slab.data_ptr(),
            acc.data_ptr() if acc is not None else None), "egtr_sgg_eval_f32")
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
             forward=None, oi=False):
    """The Visual Genome path of the reference's ``evaluate`` (evaluate_egtr.py:40-127): run the model over ``batches``
    (the reference's collate_fn format: pixel_values, pixel_mask, labels), build the candidates on the device
    (``runtime.triplet_candidates``) and score them.  Returns the reference's ``metric_dict`` keys: ``R@k`` / ``mR@k``
    of the multiple-predicate evaluator and ``(single)R@k`` / ``(single)mR@k`` of the single-predicate one.  The
    model runs through a ``GraphedForward`` when ``graphed`` (and a GPU is present); one created here is released before
    returning (``forward``: an existing ``GraphedForward`` to reuse instead, left as it is).  ``oi``: also score the
    Open Images branch (``OpenImagesRelationMetrics`` on ``triplet_candidates(mode="oi")``) and add its keys --
    w_rel_mAP, w_phr_mAP, microR@50, score, rel_mAP, phr_mAP, microR@k, and the per-image mean recalls as (oi)R@k."""
    from .runtime import GraphedForward, triplet_candidates
    if not (single or multiple or oi):
        raise ValueError("enable at least one of single / multiple / oi")
    model.eval()
    device = next(model.parameters()).device
    ev_s = SceneGraphRecall(num_rel_labels, multiple_preds=False) if single else None
    ev_m = SceneGraphRecall(num_rel_labels, multiple_preds=True) if multiple else None
    ev_oi = OpenImagesRelationMetrics(num_rel_labels) if oi else None
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
                                        pairs.data_ptr() if pairs is not None else None, pair_stride, B, M, N, R, topk,
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
