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
             forward=None):
    """The Visual Genome path of the reference's ``evaluate`` (evaluate_egtr.py:40-127): run the model over ``batches``
    (the reference's collate_fn format: pixel_values, pixel_mask, labels), build the candidates on the device
    (``runtime.triplet_candidates``) and score them.  Returns the reference's ``metric_dict`` keys: ``R@k`` / ``mR@k``
    of the multiple-predicate evaluator and ``(single)R@k`` / ``(single)mR@k`` of the single-predicate one.  The
    model runs through a ``GraphedForward`` when ``graphed`` (and a GPU is present); one created here is released before
    returning (``forward``: an existing ``GraphedForward`` to reuse instead, left as it is)."""
    from .runtime import GraphedForward, triplet_candidates
    if not (single or multiple):
        raise ValueError("enable at least one of single / multiple")
    model.eval()
    device = next(model.parameters()).device
    ev_s = SceneGraphRecall(num_rel_labels, multiple_preds=False) if single else None
    ev_m = SceneGraphRecall(num_rel_labels, multiple_preds=True) if multiple else None
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
    return metrics
