"""Seeded inputs of the Open Images relation-metrics fixture (tests/golden/oi_eval.npz, make_golden_oi_eval.py).

Model outputs (logits, pred_boxes, pred_rel, pred_connectivity) and targets in the reference's formats, built so that the
OI evaluator's edge cases occur:
  * GT objects alternate between widths W = 3v - 1 (a copy shifted right by v has bbox.pyx IoU exactly 0.5: a recall
    match, the test is >=) and W = 3v (a copy shifted by (v + 1, 1) has float32 ap_eval_rel.bbox_iou exactly 0.5: an AP
    false positive, the test is >; shifted by (v, 1) it is just above 0.5);
  * every GT triplet gets planted detections: an exact copy, often a second detection of the same GT (an FP: the GT is
    visited), sometimes the second predicate of the same pair (both enter the top 100);
  * some images hold two GT objects of one class one pixel apart, both related to the same object by the same
    predicate, and two exact copies of the first: the second copy's best GT is already visited (an FP);
  * predicates 20 .. 29 are planted on decoy pairs but never occur in the GT (AP 0 with detections); predicate 19 occurs
    in the GT but its scores are 0 everywhere (AP 0, no detections); self pairs (i, i) are planted;
  * image 3 has zero connectivity except on its planted pairs and a few pairs scaled to spo < 1e-5, so fewer than 100
    entries pass the filter and the filter drops entries inside the top 100;
  * boxes are integer pixels on a 1024 x 512 image, stored as exact binary fractions, so rescaled boxes are exact.
``check_ties`` asserts there are no ties at the top-2 boundary of a pair, among the selected entries of an image, at the
top-100 boundary, or between the confidences of one predicate class."""
import numpy as np
import torch

H_IMG, W_IMG = 512, 1024
C = 5                  # object classes (+1 no-object logit)
R = 30                 # predicates
P_GT = 19              # predicates 0 .. 18 planted and in the GT; 19 GT only (never scored); 20 .. 29 decoys only
N = 32                 # predicted objects
B = 20                 # images


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _cxcywh(box):
    x0, y0, x1, y1 = box
    return [(x0 + x1) / 2 / W_IMG, (y0 + y1) / 2 / H_IMG, (x1 - x0) / W_IMG, (y1 - y0) / H_IMG]


def _image(rng, idx):
    G = int(rng.integers(4, 7))
    gt_boxes, gt_cls, vs = [], [], []
    for g in range(G):
        v = int(rng.integers(8, 30))
        w = 3 * v - 1 if g % 2 == 0 else 3 * v
        h = int(rng.integers(20, 120))
        x0, y0 = int(rng.integers(0, W_IMG - w - 80)), int(rng.integers(0, H_IMG - h - 4))
        gt_boxes.append((x0, y0, x0 + w, y0 + h))
        gt_cls.append(int(rng.integers(0, C)))
        vs.append(v)
    dup = idx % 3 == 1
    if dup:   # GT object 1 = GT object 0 shifted by one pixel, same class
        x0, y0, x1, y1 = gt_boxes[0]
        gt_boxes[1] = (x0 + 1, y0, x1 + 1, y1)
        gt_cls[1] = gt_cls[0]
        vs[1] = vs[0]
    rels = set()
    dup_p = int(rng.integers(0, P_GT))
    if dup:
        rels |= {(0, 2, dup_p), (1, 2, dup_p)}
    T = int(rng.integers(3, 8))
    while len(rels) < T:
        s, o = (int(v) for v in rng.choice(G, 2, replace=False))
        rels.add((s, o, int(rng.integers(0, P_GT + 1))))
    rels = sorted(rels)

    objs = []   # (class, xyxy)

    def add(cls, box):
        objs.append((cls, box))
        return len(objs) - 1

    copy, near, copy2 = {}, {}, {}
    for g, (box, cls) in enumerate(zip(gt_boxes, gt_cls)):
        x0, y0, x1, y1 = box
        v = vs[g]
        copy[g] = add(cls, box)
        if (x1 - x0) % 3 == 2:     # W = 3v - 1: bbox.pyx IoU exactly 0.5
            near[g] = add(cls, (x0 + v, y0, x1 + v, y1))
        elif g % 4 == 1:           # W = 3v: float32 bbox_iou exactly 0.5
            near[g] = add(cls, (x0 + v + 1, y0 + 1, x1 + v + 1, y1 + 1))
        else:                      # just above 0.5
            near[g] = add(cls, (x0 + v, y0 + 1, x1 + v, y1 + 1))
    if dup:
        copy2[0] = add(gt_cls[0], gt_boxes[0])
    while len(objs) < N:
        x0, y0 = int(rng.integers(0, W_IMG - 40)), int(rng.integers(0, H_IMG - 40))
        add(int(rng.integers(0, C)), (x0, y0, x0 + 30, y0 + 30))
    n_real = 2 * G + len(copy2)

    planted = []   # (s, o, p), highest first
    for (s, o, p) in rels:
        if p == P_GT:
            continue
        planted.append((copy[s], copy[o], p))
        kind = int(rng.integers(0, 4))
        if kind == 0:
            planted.append((near[s], copy[o], p))                     # a second detection of this GT
        elif kind == 1:
            planted.append((copy[s], near[o], p))
        elif kind == 2:
            planted.append((copy[s], copy[o], int(rng.integers(20, R))))   # both predicates of the pair
    if dup:
        planted.append((copy2[0], copy[2], dup_p))                     # best GT already visited
    planted.append((n_real, n_real, 20 + idx % 10))                    # a self pair
    while len(planted) < 60:
        s, o = (int(v) for v in rng.choice(np.arange(n_real, N), 2, replace=False))
        planted.append((s, o, int(rng.integers(20, R))))
    rng.shuffle(planted)
    # highest score to the first planted entries, pair-predicate rows keep distinct values
    logits = rng.normal(0, 1, (N, C + 1)).astype(np.float32)
    for j, (cls, _) in enumerate(objs):
        logits[j, cls] = 3.0 + float(rng.uniform(0, 1))
    boxes = np.zeros((N, 4), np.float32)
    for j, (_, box) in enumerate(objs):
        boxes[j] = _cxcywh(box)
    rel = rng.uniform(0, 0.3, (N, N, R)).astype(np.float32)
    rel[:, :, P_GT] = 0.0
    conn = np.ones((N, N, 1), np.float32)
    for r, (s, o, p) in enumerate(planted):
        rel[s, o, p] = np.float32(0.95 - 0.006 * r + float(rng.uniform(0, 0.002)))
    if idx == 3:
        conn[:] = 0.0
        for (s, o, _) in planted[:30]:
            conn[s, o, 0] = 1.0
        for _ in range(12):
            s, o = (int(v) for v in rng.integers(0, N, 2))
            if conn[s, o, 0] == 0.0:
                conn[s, o, 0] = np.float32(float(rng.uniform(1e-6, 2e-5)))
    target_rel = np.zeros((G, G, R), np.float32)
    for (s, o, p) in rels:
        target_rel[s, o, p] = 1.0
    target = dict(class_labels=torch.tensor(gt_cls, dtype=torch.int64),
                  boxes=torch.tensor([_cxcywh(b) for b in gt_boxes], dtype=torch.float32),
                  rel=torch.from_numpy(target_rel), orig_size=torch.tensor([H_IMG, W_IMG]))
    return logits, boxes, rel, conn, target


def oi_eval_inputs(seed=83, num_images=B):
    """(outputs, targets, meta): outputs dict of [num_images, ...] tensors, targets list of target dicts."""
    rng = _rng(seed)
    L, Bx, Rl, Cn, targets = [], [], [], [], []
    for i in range(num_images):
        lg, bx, rl, cn, t = _image(rng, i)
        L.append(lg)
        Bx.append(bx)
        Rl.append(rl)
        Cn.append(cn)
        targets.append(t)
    outputs = {"logits": torch.from_numpy(np.stack(L)), "pred_boxes": torch.from_numpy(np.stack(Bx)),
               "pred_rel": torch.from_numpy(np.stack(Rl)), "pred_connectivity": torch.from_numpy(np.stack(Cn))}
    return outputs, targets, dict(num_labels=C, num_rel_labels=R)


def check_ties(pred_scores, obj_scores, pairs, prd_k=2, topk=100):
    """Assert that one image's selection does not depend on a tie rule (numpy's argsort is unstable): no tie among the
    selected entries or at the top-100 boundary, and no tie between a pair's 2nd and 3rd (or 1st and 2nd) predicate
    where the pair's 2nd entry reaches the selection."""
    srt = -np.sort(-pred_scores, axis=1)
    so = obj_scores[pairs[:, 0]] * obj_scores[pairs[:, 1]]
    spo = (so[:, None] * srt[:, :prd_k]).ravel()
    spo = spo[spo > 1e-5]
    top = -np.sort(-spo)
    sel = top[:topk]
    assert len(np.unique(sel)) == len(sel), "tie among the selected entries"
    if len(top) > topk:
        assert top[topk - 1] != top[topk], "tie at the top-100 boundary"
    thr = max(sel[-1] if len(sel) else np.inf, np.float32(1e-5))
    reach = so * srt[:, 1] >= thr
    assert not (reach & (srt[:, 1] == srt[:, 2])).any(), "tie at the top-2 boundary"
    assert not (reach & (srt[:, 0] == srt[:, 1])).any(), "tie between a pair's two best predicates"
