"""A literal loop restatement of pycocotools COCOeval(iouType="bbox") evaluateImg / accumulate / summarize in plain
Python and numpy, written apart from the product's vectorised host path (egtr_amd.evaluation.coco_match_host /
coco_accumulate_host) so that the two check each other.  Not a test module.

Images are lists: dets [(score fp32, label, (x0, y0, x1, y1) fp32)], gts [((x, y, w, h) fp64, area, iscrowd, label)]."""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNGS = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]


def bb_iou(d, g, crowd):
    """maskApi bbIou of one pair (xywh, Python floats = C doubles)."""
    da = d[2] * d[3]
    ga = g[2] * g[3]
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = da if crowd else da + ga - i
    return i / u


def to_coco_dets(dets, num_classes):
    """CocoEvaluator.prepare_for_coco_detection + loadRes: fp32 xywh (w = x1 - x0 in fp32) as doubles, area w * h;
    labels outside [0, num_classes) dropped (an unknown category)."""
    out = []
    for score, label, box in dets:
        if not 0 <= label < num_classes:
            continue
        x0, y0, x1, y1 = (np.float32(v) for v in box)
        bb = [float(x0), float(y0), float(np.float32(x1 - x0)), float(np.float32(y1 - y0))]
        out.append({"score": float(np.float32(score)), "category_id": int(label), "bbox": bb, "area": bb[2] * bb[3]})
    return out


def evaluate_img(dt, gt, a_rng, max_det):
    """COCOeval.evaluateImg of one (image, category): returns None or the dict accumulate reads."""
    if len(gt) == 0 and len(dt) == 0:
        return None
    gt = [dict(g) for g in gt]
    for g in gt:
        g["_ignore"] = 1 if (g["iscrowd"] or g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0
    gtind = np.argsort([g["_ignore"] for g in gt], kind="mergesort")
    gt = [gt[i] for i in gtind]
    dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
    dt = [dt[i] for i in dtind[0:max_det]]
    iscrowd = [int(g["iscrowd"]) for g in gt]
    ious = [[bb_iou(d["bbox"], g["bbox"], iscrowd[j]) for j, g in enumerate(gt)] for d in dt]
    T, G, D = len(IOU_THRS), len(gt), len(dt)
    gtm = np.zeros((T, G))
    dtm = np.zeros((T, D))
    gt_ig = np.array([g["_ignore"] for g in gt])
    dt_ig = np.zeros((T, D))
    if G and D:
        for tind, t in enumerate(IOU_THRS):
            for dind, d in enumerate(dt):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind, g in enumerate(gt):
                    if gtm[tind, gind] > 0 and not iscrowd[gind]:
                        continue
                    if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                        break
                    if ious[dind][gind] < iou:
                        continue
                    iou = ious[dind][gind]
                    m = gind
                if m == -1:
                    continue
                dt_ig[tind, dind] = gt_ig[m]
                dtm[tind, dind] = 1
                gtm[tind, m] = 1
    a = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] for d in dt]).reshape((1, len(dt)))
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
    return {"dtMatches": dtm, "dtScores": [d["score"] for d in dt], "gtIgnore": gt_ig, "dtIgnore": dt_ig}


def evaluate(images, num_classes):
    """evaluate + accumulate over ``images`` [(dets, gts)] in image order: (precision [T, R, K, A, M], recall [T, K, A, M],
    eval_imgs {(k, a, img): dict})."""
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), num_classes, len(AREA_RNGS), len(MAX_DETS)
    eval_imgs = {}
    for i, (dets, gts) in enumerate(images):
        cd = to_coco_dets(dets, num_classes)
        for k in range(K):
            dt = [d for d in cd if d["category_id"] == k]
            gt = [{"bbox": [float(v) for v in g[0]], "area": float(g[1]), "iscrowd": int(g[2])} for g in gts
                  if int(g[3]) == k]
            for a, rng in enumerate(AREA_RNGS):
                eval_imgs[(k, a, i)] = evaluate_img(dt, gt, rng, MAX_DETS[-1])
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k in range(K):
        for a in range(A):
            E = [eval_imgs[(k, a, i)] for i in range(len(images))]
            E = [e for e in E if e is not None]
            if len(E) == 0:
                continue
            for m, max_det in enumerate(MAX_DETS):
                dt_scores = np.concatenate([e["dtScores"][0:max_det] for e in E])
                inds = np.argsort(-dt_scores, kind="mergesort")
                dtm = np.concatenate([e["dtMatches"][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dtIgnore"][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp = np.array(tp)
                    fp = np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    q = q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds_r = np.searchsorted(rc, REC_THRS, side="left")
                    try:
                        for ri, pi in enumerate(inds_r):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
    return precision, recall, eval_imgs


def summarize(precision, recall):
    """COCOeval.summarize's 12 stats (the same order as egtr_amd.evaluation.COCO_STATS)."""
    def s(ap=1, iou_thr=None, area="all", max_dets=100):
        aind = ["all", "small", "medium", "large"].index(area)
        mind = MAX_DETS.index(max_dets)
        if ap == 1:
            x = precision
            if iou_thr is not None:
                x = x[np.where(iou_thr == IOU_THRS)[0]]
            x = x[:, :, :, aind, mind]
        else:
            x = recall
            if iou_thr is not None:
                x = x[np.where(iou_thr == IOU_THRS)[0]]
            x = x[:, :, aind, mind]
        return -1 if len(x[x > -1]) == 0 else np.mean(x[x > -1])
    return [s(1), s(1, .5), s(1, .75), s(1, area="small"), s(1, area="medium"), s(1, area="large"),
            s(0, max_dets=1), s(0, max_dets=10), s(0), s(0, area="small"), s(0, area="medium"), s(0, area="large")]
