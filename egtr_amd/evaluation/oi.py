"""The Open Images relation metrics (``OpenImagesRelationMetrics``; oi_eval.py eval_rel_results, ap_eval_rel.py;
csrc/oi_eval.hip) reproduce these reference semantics:
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
"""
import ctypes

import torch

from .. import _lib
from ._common import (FlatAccumulator, StagingRing, _tensor, backend_device, check_gt_predicates, check_ks,
                      first_ranks_host, gather_records, gt_entry, upload_relation_gt)

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


class OpenImagesRelationMetrics(FlatAccumulator):
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
        ks = check_ks(num_rel_labels, ks)
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
        self._ring = StagingRing()
        self.reset()

    # ---- state -----------------------------------------------------------------------------------------------------
    def reset(self, device=None):
        self._reset_acc(device)
        self._batches = []         # (p [B, topk], score [B, topk], tp uint8 [2, B, topk], valid bool [B, topk]) per update

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
        dev = backend_device(group)
        if self.acc is None:
            self._acc_on(dev)
        acc = self.acc.to(dev)
        dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=group)
        p, s, tp = (x.to(dev) for x in self._records())
        # one float64 row set per rank: p, score (exact in float64), tp_rel, tp_phr
        cat = gather_records(torch.cat([p.double()[None], s.double()[None], tp.double()]), group)
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
            check_gt_predicates(g, self.num_rel)
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
        for r in rows:          # image order, like eval_fold
            acc.add_(r)
        self._batches.append((p_out, s_out, tp_out, valid))
        self.last_detections = dets
        self.last_rows = torch.stack(rows)

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
        gt = upload_relation_gt(self._ring, gts, device)
        slab = torch.empty(B, self.width, dtype=torch.float64, device=device)
        tp = torch.empty(2, B, topk, dtype=torch.uint8, device=device)
        ks = (ctypes.c_int * nk)(*self.ks)
        _lib.check(h.egtr_oi_match_f32(
            stream, sop.data_ptr(), count.data_ptr(), B, topk, boxes.data_ptr(), classes.data_ptr(), N, self.num_rel,
            _lib.ptr(gt.rels), gt.rel_off.data_ptr(), gt.T, _lib.ptr(gt.boxes), _lib.ptr(gt.classes),
            gt.box_off.data_ptr(), gt.G, ks, nk, tp.data_ptr(), slab.data_ptr(), acc.data_ptr()), "egtr_oi_match_f32")
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
