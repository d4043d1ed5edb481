"""Seeded inputs of the scene-graph evaluator fixture (tests/golden/sgg_eval.npz, make_golden_sgg_eval.py).

Model outputs (logits, pred_boxes, pred_rel, pred_connectivity) and targets in the reference's formats, designed so the
metrics mean something:
  * every predicted object's logit row is a permutation of the same vector, so all object scores are equal and the
    candidate order is the order of the PLANTED relation scores: slot r (r = 0 .. S-1) gets 0.9 * (1 - 0.002 r) at its
    (s, o, p), everything else is uniform in [0, 0.3) -- strictly distinct top scores, relative gaps 2e-3, and more than
    100 distinct planted pairs, so both top-100 lists (triplets and pairs) end inside the planted slots;
  * each GT triplet gets an exact-copy candidate at a rank drawn from [0, 20), [20, 50), [50, 100), [100, S) (cut off by
    the top-100) or none, plus decoys at random ranks: wrong subject class, wrong object class, wrong predicate, a subject
    box with IoU exactly 0.5 (a match: the test is >=) and one just below it;
  * some images hold two GT objects of one class with near-identical boxes related to the same object by the same
    predicate, so one candidate matches two GT triplets; the last three predicates never occur (mR's NaN path);
  * boxes are integer pixels on a 1024 x 512 image, stored as normalised cxcywh that are exact binary fractions, so the
    rescaled boxes (host or device, float32) are exact.
``chain=True`` moves the planted IoUs off 0.5 (0.519 / 0.463 instead of 0.5 / 0.481) for the device chain test, whose
scores differ from the host's in the last bits."""
import numpy as np
import torch

H_IMG, W_IMG = 512, 1024
C, R = 20, 12          # object classes (+1 no-object logit), predicates
R_USED = R - 3         # predicates R-3 .. R-1 never occur in the GT
N = 64                 # predicted objects
S = 140                # planted slots
B = 16                 # images


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _cxcywh(box):
    x0, y0, x1, y1 = box
    return [(x0 + x1) / 2 / W_IMG, (y0 + y1) / 2 / H_IMG, (x1 - x0) / W_IMG, (y1 - y0) / H_IMG]


def _image(rng, chain, dup):
    G = int(rng.integers(6, 11))
    gt_boxes, gt_cls = [], []
    for _ in range(G):
        d = int(rng.integers(10, 50))
        a, b = 3 * d, int(rng.integers(20, 150))
        x0, y0 = int(rng.integers(0, W_IMG - a - 80)), int(rng.integers(0, H_IMG - b - 2))
        gt_boxes.append((x0, y0, x0 + a - 1, y0 + b - 1))
        gt_cls.append(int(rng.integers(0, C - 1)))
    if dup:   # GT object 1 = GT object 0 shifted by one pixel, same class
        x0, y0, x1, y1 = gt_boxes[0]
        gt_boxes[1] = (x0 + 1, y0, x1 + 1, y1)
        gt_cls[1] = gt_cls[0]
    rels = set()
    if dup:
        p = int(rng.integers(0, R_USED))
        rels |= {(0, 2, p), (1, 2, p)}
    T = int(rng.integers(4, 13))
    while len(rels) < T:
        s, o = (int(v) for v in rng.choice(G, 2, replace=False))
        rels.add((s, o, int(rng.integers(0, R_USED))))
    rels = sorted(rels)

    # predicted objects: per GT object an exact copy, a half-IoU copy (shifted right by a/3 px: IoU = 0.5 exactly), a
    # just-below copy, a wrong-class copy; then decoy objects of class C - 1 (never in the GT)
    objs = []   # (class, xyxy)

    def add(cls, box):
        objs.append((cls, box))
        return len(objs) - 1

    copy, half, below, wrong = {}, {}, {}, {}
    for g, (box, cls) in enumerate(zip(gt_boxes, gt_cls)):
        x0, y0, x1, y1 = box
        d = (x1 - x0 + 1) // 3
        dh, db = (d - 1, d + 2) if chain else (d, d + 1)
        copy[g] = add(cls, box)
        half[g] = add(cls, (x0 + dh, y0, x1 + dh, y1))
        below[g] = add(cls, (x0 + db, y0, x1 + db, y1))
        wrong[g] = add((cls + 1) % (C - 1), box)
    while len(objs) < N:
        x0, y0 = int(rng.integers(0, W_IMG - 40)), int(rng.integers(0, H_IMG - 40))
        add(C - 1, (x0, y0, x0 + 30, y0 + 30))

    slots = [None] * S
    free = list(range(S))

    def place(lo, hi, trip):
        cand = [r for r in free if lo <= r < hi]
        if not cand or trip in slots:
            return
        r = int(rng.choice(cand))
        free.remove(r)
        slots[r] = trip

    for (s, o, p) in rels:
        band = int(rng.integers(0, 5))
        lo, hi = [(0, 20), (20, 50), (50, 100), (100, S), (0, 0)][band]
        place(lo, hi, (copy[s], copy[o], p))
        for _ in range(int(rng.integers(0, 4))):
            kind = int(rng.integers(0, 5))
            trip = [(wrong[s], copy[o], p), (copy[s], wrong[o], p), (copy[s], copy[o], (p + 1) % R_USED),
                    (half[s], copy[o], p), (below[s], copy[o], p)][kind]
            place(0, S, trip)
    decoys = list(range(4 * G, N))
    used_pairs = {(t[0], t[1]) for t in slots if t is not None}
    for r in free:   # fillers: distinct decoy pairs, never a match
        while True:
            s, o = (int(v) for v in rng.choice(decoys, 2, replace=False))
            if (s, o) not in used_pairs:
                break
        used_pairs.add((s, o))
        slots[r] = (s, o, int(rng.integers(0, R)))

    logits = np.zeros((N, C + 1), np.float32)
    logits[:, C] = -1.0
    boxes = np.zeros((N, 4), np.float32)
    for j, (cls, box) in enumerate(objs):
        logits[j, cls] = 4.0
        boxes[j] = _cxcywh(box)
    rel = rng.uniform(0, 0.3, (N, N, R)).astype(np.float32)
    for r, (s, o, p) in enumerate(slots):
        rel[s, o, p] = np.float32(0.9 * (1 - 0.002 * r))
    target_rel = np.zeros((G, G, R), np.float32)
    for (s, o, p) in rels:
        target_rel[s, o, p] = 1.0
    target = dict(class_labels=torch.tensor(gt_cls, dtype=torch.int64),
                  boxes=torch.tensor([_cxcywh(b) for b in gt_boxes], dtype=torch.float32),
                  rel=torch.from_numpy(target_rel), orig_size=torch.tensor([H_IMG, W_IMG]))
    return logits, boxes, rel, target


def sgg_eval_inputs(seed=71, chain=False, num_images=B):
    """(outputs, targets, meta): outputs dict of [num_images, ...] tensors, targets list of target dicts."""
    rng = _rng(seed)
    L, Bx, Rl, targets = [], [], [], []
    for i in range(num_images):
        lg, bx, rl, t = _image(rng, chain, dup=(i % 4 == 1))
        L.append(lg)
        Bx.append(bx)
        Rl.append(rl)
        targets.append(t)
    outputs = {"logits": torch.from_numpy(np.stack(L)), "pred_boxes": torch.from_numpy(np.stack(Bx)),
               "pred_rel": torch.from_numpy(np.stack(Rl)), "pred_connectivity": torch.ones(num_images, N, N, 1)}
    return outputs, targets, dict(num_labels=C, num_rel_labels=R)
