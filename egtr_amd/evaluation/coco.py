"""The COCO box-detection metrics (``CocoDetectionMetrics``; pycocotools COCOeval(iouType="bbox") as the reference's
CocoEvaluator runs it, lib/evaluation/coco_eval.py; csrc/coco_eval.hip) reproduce evaluateImg's greedy matching at ten
IoU thresholds and four area ranges, accumulate's precision / recall tables and summarize's 12 stats.  Image order is
update order (the reference sorts by image id); a match is a flag, not a GT id (pycocotools ignores a match to a GT whose
annotation id is 0); ``evaluate(coco=True)`` adds the reference's "AP50".
"""
import collections
import ctypes

import numpy as np
import torch

from .. import _lib
from ._common import StagingRing, _tensor, backend_device, copy_staged, gather_records, placed, rescale_bboxes

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


# The COCO GT layout, the byte contract with coco_eval.hip:
#   int64 [offsets B+1 | labels G], then fp64 [boxes 4G | area G], then uint8 crowd G
# labels: the int64 index where that section starts; f64_at / crowd_at: the byte offsets of the fp64 part and the flags.
CocoLayout = collections.namedtuple("CocoLayout", "G labels f64_at crowd_at nbytes")


def coco_layout(g):
    """Sizes and section offsets of the COCO GT layout for a batch of normalised GT dicts."""
    B, G = len(g), sum(x["labels"].shape[0] for x in g)
    n64 = B + 1 + G
    return CocoLayout(G, B + 1, 8 * n64, 8 * n64 + 40 * G, 8 * n64 + 40 * G + G)


def pack_coco_gt(g, lay, buf):
    """Write the batch's ragged GT into the first ``lay.nbytes`` of the uint8 host buffer ``buf`` (pinned or not)."""
    G = lay.G
    i64 = buf[:lay.f64_at].view(torch.int64)
    f64 = buf[lay.f64_at:lay.crowd_at].view(torch.float64)
    i64[:lay.labels] = torch.tensor([0] + [x["labels"].shape[0] for x in g], dtype=torch.int64).cumsum(0)
    if G:
        i64[lay.labels:] = torch.cat([x["labels"] for x in g])
        f64[:4 * G] = torch.cat([x["boxes"] for x in g]).reshape(-1)
        f64[4 * G:] = torch.cat([x["area"] for x in g])
        buf[lay.crowd_at:lay.nbytes] = torch.cat([x["iscrowd"] for x in g])


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
        self._ring = StagingRing()
        self.reset()

    # ---- state -----------------------------------------------------------------------------------------------------
    def reset(self):
        self.npig = None           # int32 [K, A] on the device of the first update
        self._batches = []         # (label int32 [B, D], score fp32 [B, D], rank int32 [B, D], bits int64 [B, D, 2])
        self._n_images = 0
        self._result = None
        self.last_matches = None

    def _npig_on(self, device):
        self.npig = placed(self.npig, device, (self.num_classes, len(COCO_AREA_RNGS)), torch.int32)
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
        dev = backend_device(group)
        K, A = self.num_classes, len(COCO_AREA_RNGS)
        home = self.npig.device if self.npig is not None else dev
        acc = torch.zeros(K * A + 1, dtype=torch.int64, device=dev)
        if self.npig is not None:
            acc[:K * A] = self.npig.reshape(-1).to(dev).long()
        acc[K * A] = self._n_images
        dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=group)
        label, score, rank, bits = (x.to(dev) for x in self._records())
        # one int64 row set per rank: label, score bits, rank, match bits, ignore bits
        cat = gather_records(torch.cat([label.long()[None], score.contiguous().view(torch.int32).long()[None],
                                        rank.long()[None], bits.t()]), group)
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
        lay = coco_layout(g)
        slot = self._ring.slot(lay.nbytes)
        pack_coco_gt(g, lay, slot[0])
        dev = copy_staged(slot, lay.nbytes, device)
        G = lay.G
        d64 = dev[:lay.f64_at].view(torch.int64)
        df = dev[lay.f64_at:lay.crowd_at].view(torch.float64)
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
            dev[lay.crowd_at:].data_ptr() if G else None, d64[lay.labels:].data_ptr() if G else None, d64.data_ptr(), G,
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
