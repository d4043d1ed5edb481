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

import numpy as np
import torch

from .. import _lib
from ..kernels.statistics import sgg_zero_shot
from ._common import (_MAX_CAND, FlatAccumulator, StagingRing, backend_device, check_gt_predicates, check_ks,
                      first_ranks_host, gt_entry, numpy_argmax, placed, seen_bits_host, upload_relation_gt)


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


class SceneGraphRecall(FlatAccumulator):
    """R@k (and per-predicate R@k, mR@k) of the reference's BasicSceneGraphEvaluator in sgdet mode.

    ``multiple_preds=False``: graph-constrained (the reference's "single" evaluator: candidates [K, 2] + rel_scores
    [K, R], predicate = argmax of the row); ``True``: candidates [K, 3].  All metrics live in ONE flat float64 tensor
    ``acc`` (sums of per-image recalls, image counts, skipped count; see csrc/sgg_eval.hip for the layout), on the device
    of the first ``update`` -- ``merge`` / ``all_reduce`` add it.

    ``train_counts``: also accumulate the ZERO-SHOT recall -- the recall over the GT triplets whose
    (subject class, object class, predicate) has count 0 in the training set.  A ``RelationStatistics``, an ``fg_matrix``
    array [C1, C1, R], or a ``seen_bits`` tensor (then with ``train_num_labels`` = C1 - 1); read once, here.  Its state is
    the separate flat float64 ``zs_acc`` [len(ks) + 2]: sums of per-image zero-shot recalls, the number of images with a
    zero-shot GT triplet, the number of such triplets.  ``acc`` and ``width`` are the same with or without it."""

    def __init__(self, num_rel_labels, ks=(20, 50, 100), multiple_preds=False, iou_thresh=0.5, keep_per_image=False,
                 train_counts=None, train_num_labels=None):
        ks = check_ks(num_rel_labels, ks)
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
        self._ring = StagingRing()
        self._seen_bits, self._zs_classes = None, 0
        if train_counts is not None:
            self._read_train_counts(train_counts, train_num_labels)
        self.reset()

    def _read_train_counts(self, train_counts, train_num_labels):
        R = self.num_rel
        if callable(getattr(train_counts, "seen_bits", None)):       # a RelationStatistics
            if train_counts.shape[2] != R:
                raise ValueError(f"train_counts counts {train_counts.shape[2]} predicates, the evaluator {R}")
            bits, C1 = train_counts.seen_bits(), train_counts.shape[0]
        elif torch.is_tensor(train_counts) and train_counts.dim() == 1:
            if train_num_labels is None:
                raise ValueError("a seen_bits tensor needs train_num_labels")
            bits, C1 = train_counts.long().contiguous(), int(train_num_labels) + 1
        else:
            fg = train_counts if torch.is_tensor(train_counts) else torch.from_numpy(np.ascontiguousarray(train_counts))
            if fg.dim() != 3 or fg.shape[0] != fg.shape[1] or fg.shape[2] != R:
                raise ValueError(f"an fg_matrix must be [C1, C1, {R}], got {tuple(fg.shape)}")
            bits, C1 = seen_bits_host(fg.cpu()), fg.shape[0]
        if bits.numel() < (C1 * C1 * R + 63) // 64:
            raise ValueError(f"seen_bits holds {bits.numel()} words, {C1} x {C1} x {R} bits need more")
        self._seen_bits, self._zs_classes = bits, C1

    # ---- state -----------------------------------------------------------------------------------------------------
    def reset(self, device=None):
        self._reset_acc(device)
        self._per_image = []       # slab columns [B, nk + 2] (recalls, counted, skipped) per update
        self.zs_acc = None if device is None or self._seen_bits is None else torch.zeros(
            len(self.ks) + 2, dtype=torch.float64, device=device)
        self._per_image_zs = []    # zero-shot rows [B, nk + 2] per update

    def _zs_on(self, device):
        """``zs_acc`` (placed like ``acc``) with the bitset beside it."""
        self.zs_acc = placed(self.zs_acc, device, len(self.ks) + 2, torch.float64)
        if self._seen_bits.device != device:
            self._seen_bits = self._seen_bits.to(device)
        return self.zs_acc

    def merge(self, other):
        """Add another evaluator's accumulators (same ks / num_rel_labels) into this one."""
        if (other.ks, other.num_rel, other.multiple_preds) != (self.ks, self.num_rel, self.multiple_preds):
            raise ValueError("merge needs evaluators with the same ks, num_rel_labels and mode")
        if other.acc is not None:
            self._acc_on(other.acc.device).add_(other.acc)
        self._per_image += other._per_image
        if other.zs_acc is not None:
            self.zs_acc = placed(self.zs_acc, other.zs_acc.device, len(self.ks) + 2, torch.float64).add_(other.zs_acc)
        self._per_image_zs += other._per_image_zs
        return self

    def all_reduce(self, group=None):
        """Sum the accumulators over the ranks of ``group`` (one collective on the flat tensor).  No-op when
        torch.distributed is not initialised."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return self
        if self.acc is None:
            self._acc_on(backend_device(group))
        dist.all_reduce(self.acc, op=dist.ReduceOp.SUM, group=group)
        if self._seen_bits is not None:   # every rank was constructed alike
            dist.all_reduce(self._zs_on(self.acc.device), op=dist.ReduceOp.SUM, group=group)
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
            check_gt_predicates(g, self.num_rel)
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

    def _zero_shot_row(self, fr, g, K):
        """One zero-shot row (float64 [nk + 2]) from the first ranks of an image, as sgg_zero_shot writes it."""
        nk, R, C1 = len(self.ks), self.num_rel, self._zs_classes
        row = torch.zeros(nk + 2, dtype=torch.float64)
        rels = g["gt_relations"]
        if rels.shape[0] == 0:
            return row
        cs, co = g["gt_classes"][rels[:, 0]], g["gt_classes"][rels[:, 1]]
        ok = (cs >= 0) & (cs < C1) & (co >= 0) & (co < C1)
        bit = ((cs * C1 + co) * R + rels[:, 2]).clamp(0, C1 * C1 * R - 1)
        zs = ok & (((self._seen_bits[bit >> 6] >> (bit & 63)) & 1) == 0)
        n = int(zs.sum())
        if n:
            row[:nk] = torch.tensor([float(int((zs & (fr < min(k, K))).sum())) / float(n) for k in self.ks],
                                    dtype=torch.float64)
            row[nk], row[nk + 1] = 1.0, float(n)
        return row

    _first_ranks = staticmethod(first_ranks_host)     # the host matching; a subclass with another box test replaces it

    def _update_host(self, candidates, gts):
        acc = self._acc_on(torch.device("cpu"))
        zs_acc = None if self._seen_bits is None else self._zs_on(torch.device("cpu"))
        rows, zs_rows = [], []
        for c, g in zip(candidates, gts):
            inds = c["pred_rel_inds"].long()
            if self.multiple_preds:
                rels = inds[:, :3]
            else:
                rels = torch.cat([inds[:, :2], numpy_argmax(c["rel_scores"].float())[:, None]], 1)
            fr = self._first_ranks(rels, c["pred_boxes"].float(), c["pred_classes"].long(), g["gt_relations"],
                                   g["gt_boxes"], g["gt_classes"], self.iou_thresh)
            rows.append(self._image_row(fr, g["gt_relations"], rels.shape[0]))
            if zs_acc is not None:
                zs_rows.append(self._zero_shot_row(fr, g, rels.shape[0]))
        for r in rows:          # image order, like eval_fold
            acc.add_(r)
        for r in zs_rows:
            zs_acc.add_(r)
        if self.keep_per_image:
            self._per_image.append(torch.stack(rows)[:, :len(self.ks) + 2])
            if zs_rows:
                self._per_image_zs.append(torch.stack(zs_rows))

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
        self._staged = (inds, scores, boxes, classes, upload_relation_gt(self._ring, gts, device))
        slab = self._launch(acc)
        if self.keep_per_image:
            self._per_image.append(slab[:, :len(self.ks) + 2].clone())
        if self._seen_bits is not None:   # right behind the matching pass, on its stream: reads the first ranks it left
            zs_acc = self._zs_on(device)
            with torch.cuda.device(device):
                zs_slab = sgg_zero_shot(self.last_first_rank, self._staged[4], B, inds.shape[1], self._zs_classes,
                                        self.num_rel, self._seen_bits, self.ks, zs_acc)
            if self.keep_per_image:
                self._per_image_zs.append(zs_slab)

    def _launch(self, acc):
        """egtr_sgg_eval_f32 on the inputs the last device update staged (``_staged``); returns the slab."""
        inds, scores, boxes, classes, gt = self._staged
        B, K, N = inds.shape[0], inds.shape[1], boxes.shape[1]
        slab = torch.empty(B, self.width, dtype=torch.float64, device=boxes.device)
        first_rank = torch.empty(max(gt.T, 1), dtype=torch.int32, device=boxes.device)
        ks = (ctypes.c_int * len(self.ks))(*self.ks)
        stream = torch.cuda.current_stream(boxes.device).cuda_stream
        _lib.check(_lib.lib().egtr_sgg_eval_f32(
            stream, inds.data_ptr(), inds.shape[2], _lib.ptr(scores), boxes.data_ptr(),
            classes.data_ptr(), B, K, N, self.num_rel, _lib.ptr(gt.rels), gt.rel_off.data_ptr(), gt.T,
            _lib.ptr(gt.boxes), _lib.ptr(gt.classes), gt.box_off.data_ptr(), gt.G, ks, len(self.ks), self.iou_thresh,
            first_rank.data_ptr(), slab.data_ptr(), _lib.ptr(acc)), "egtr_sgg_eval_f32")
        self.last_first_rank = first_rank[:gt.T]
        return slab

    # ---- results (one synchronisation each) --------------------------------------------------------------------------
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

    def _host_zs(self):
        if self._seen_bits is None:
            raise RuntimeError("construct the evaluator with train_counts=...")
        return torch.zeros(len(self.ks) + 2, dtype=torch.float64) if self.zs_acc is None else self.zs_acc.cpu()

    def zero_shot(self):
        """{"zR@k": mean per-image zero-shot recall} over the images that have a zero-shot GT triplet; NaN without one."""
        a = self._host_zs().tolist()
        nk = len(self.ks)
        return {f"zR@{k}": self._mean(a[j], a[nk]) for j, k in enumerate(self.ks)}

    @property
    def n_zero_shot_images(self):
        return int(self._host_zs()[len(self.ks)])

    @property
    def n_zero_shot_triplets(self):
        return int(self._host_zs()[len(self.ks) + 1])

    def per_image_zero_shot(self):
        """Per-image zero-shot recalls [n, len(ks)] (float64, host) of the images that have a zero-shot GT triplet, in
        update order."""
        if not self.keep_per_image:
            raise RuntimeError("construct the evaluator with keep_per_image=True")
        self._host_zs()
        nk = len(self.ks)
        if not self._per_image_zs:
            return torch.zeros(0, nk, dtype=torch.float64)
        rows = torch.cat([r.cpu() for r in self._per_image_zs])
        return rows[rows[:, nk] == 1][:, :nk]

    def per_image(self):
        """Per-image recalls [n_images, len(ks)] (float64, host) of the images that were not skipped, in update order."""
        if not self.keep_per_image:
            raise RuntimeError("construct the evaluator with keep_per_image=True")
        nk = len(self.ks)
        if not self._per_image:
            return torch.zeros(0, nk, dtype=torch.float64)
        rows = torch.cat([r.cpu() for r in self._per_image])
        return rows[rows[:, nk + 1] == 0][:, :nk]
