"""Seeded inputs of the phrase- / predicate-detection fixture (tests/golden/vrd_eval.npz, make_golden_vrd_eval.py).

Targets in the reference's format plus, per image, the two ``pred_entry`` dicts the VRD evaluators read:
  * phrdet: N predicted objects -- per GT object an exact copy, copies shifted right by 1/3 of the width (IoU exactly 0.5
    with the GT box), by 1/3 + 1 px (just below) and by 2/3 (IoU 0.2); wrong-class copies of the first GT objects and
    decoy objects fill the rest -- and K
    ranked (s, o, p) candidates: for each GT triplet a candidate built from random variants of its two objects at a rank
    drawn from [0, 20), [20, 50), [50, K) or none (the union boxes of shifted parts overlap the GT union far more than the
    parts overlap each other, so phrdet matches where sgdet does not), wrong-predicate / wrong-class decoys and random
    fillers.  Scores descend strictly; object scores are 1.
  * preddet: K (s, o) pairs of GT OBJECT indices with uniform random float32 scores [K, R].  Row 0 is a pair that is no
    GT pair, every GT pair occurs (first occurrence at a random row, one of them at row 64 where K allows, later rows
    repeat earlier pairs) except that every third image drops ONE GT pair, which then falls back to row 0.  GT pairs are
    distinct inside an image, so no two list entries carry the same score (the generator asserts it) and numpy's unstable
    argsort has one answer.  One image has no candidates at all.
Boxes are integer pixels on a 1024 x 512 image, stored as normalised cxcywh that are exact binary fractions."""
import numpy as np
import torch

from sgg_eval_inputs import C, H_IMG, W_IMG, _cxcywh, _rng

R = 12                 # predicates; the last three never occur in the GT
R_USED = R - 3
N = 48                 # predicted objects (phrdet)
KS_OF_IMAGE = (100,) * 8 + (65,) * 4          # candidates per image, both protocols
NINE = 0               # the image with exactly 9 GT triplets
NO_CAND = 5            # the image without preddet candidates


def _image(rng, i, K):
    G = int(rng.integers(9, 12)) if K > 90 else int(rng.integers(8, 10))   # G (G - 1) > 56, and > 90 where K = 100
    gt_boxes, gt_cls = [], []
    for _ in range(G):
        d = int(rng.integers(10, 40))
        a, b = 3 * d, int(rng.integers(20, 150))
        x0, y0 = int(rng.integers(0, W_IMG - 2 * a - 2)), int(rng.integers(0, H_IMG - b - 2))
        gt_boxes.append((x0, y0, x0 + a - 1, y0 + b - 1))
        gt_cls.append(int(rng.integers(0, C - 1)))
    all_pairs = [(s, o) for s in range(G) for o in range(G) if s != o]
    T = 9 if i == NINE else int(rng.integers(3, 11))
    gt_pairs = [all_pairs[j] for j in rng.choice(len(all_pairs), T, replace=False)]      # distinct pairs
    rels = sorted((s, o, int(rng.integers(0, R_USED))) for s, o in gt_pairs)

    # ---- phrdet ------------------------------------------------------------------------------------------------------
    objs = []
    variants, wrong = {}, {}
    for g, (box, cls) in enumerate(zip(gt_boxes, gt_cls)):
        x0, y0, x1, y1 = box
        d = (x1 - x0 + 1) // 3
        variants[g] = []
        for dx in (0, d, d + 1, 2 * d):
            objs.append((cls, (x0 + dx, y0, x1 + dx, y1)))
            variants[g].append(len(objs) - 1)
    for g in range(min(G, (N - len(objs)) // 2)):
        objs.append(((gt_cls[g] + 1) % (C - 1), gt_boxes[g]))
        wrong[g] = len(objs) - 1
    while len(objs) < N:
        x0, y0 = int(rng.integers(0, W_IMG - 40)), int(rng.integers(0, H_IMG - 40))
        objs.append((C - 1, (x0, y0, x0 + 30, y0 + 30)))
    assert len(objs) == N
    slots = [None] * K
    free = list(range(K))

    def place(lo, hi, trip):
        cand = [r for r in free if lo <= r < hi]
        if cand:
            r = int(rng.choice(cand))
            free.remove(r)
            slots[r] = trip

    for n, (s, o, p) in enumerate(rels):
        lo, hi = [(0, 20), (20, 50), (50, K), (0, 0)][int(rng.integers(0, 4))]
        if i >= 8 and n == 0:
            lo, hi = 64, 65          # the last candidate of a K = 65 image: lane 0 of the second 64-candidate step
        vs, vo = (int(v) for v in rng.integers(0, 4, 2))
        place(lo, hi, (variants[s][vs], variants[o][vo], p))
        for _ in range(int(rng.integers(0, 3))):
            kind = int(rng.integers(0, 4))
            ws, wo = wrong.get(s, variants[s][3]), wrong.get(o, variants[o][3])
            place(0, K, [(ws, variants[o][0], p), (variants[s][0], wo, p), (variants[s][0], variants[o][0], (p + 1) % R),
                         (variants[s][3], variants[o][3], p)][kind])
    for r in free:
        s, o = (int(v) for v in rng.choice(N, 2, replace=False))
        slots[r] = (s, o, int(rng.integers(0, R)))
    boxes = np.array([b for _, b in objs], np.float32)
    phr = dict(pred_boxes=boxes, pred_classes=np.array([c for c, _ in objs], np.int64),
               obj_scores=np.ones(N, np.float32), pred_rel_inds=np.array(slots, np.int64),
               rel_scores=(0.9 * (1 - 0.002 * np.arange(K))).astype(np.float32))

    # ---- preddet -----------------------------------------------------------------------------------------------------
    if i == NO_CAND:
        prd = dict(pred_rel_inds=np.zeros((0, 2), np.int64), rel_scores=np.zeros((0, R), np.float32))
    else:
        present = list(gt_pairs)
        if i % 3 == 2:
            present.pop(int(rng.integers(0, len(present))))          # one GT pair without a candidate: row 0 is chosen
        others = [pr for pr in all_pairs if pr not in gt_pairs]
        rows = [None] * K
        rows[0] = others.pop(int(rng.integers(0, len(others))))
        pool = present + others
        order = [pool[j] for j in rng.permutation(len(pool))][:K - 1]
        for pr in present:                                           # every kept GT pair is in the list
            if pr not in order:
                order[int(rng.integers(0, len(order)))] = pr
        order = list(dict.fromkeys(order))
        for pr in present:
            assert pr in order
        if K > 64:                                                   # first occurrence of one GT pair at row 64
            order.remove(present[0])
        first = iter(order)
        for r in range(1, K):
            if r == 64 and K > 64:
                rows[r] = present[0]
                continue
            nxt = next(first, None)
            rows[r] = nxt if nxt is not None else rows[int(rng.integers(0, r))]   # a repeat of an earlier row
        if K > 64:
            assert rows.index(present[0]) == 64
        prd = dict(pred_rel_inds=np.array(rows, np.int64), rel_scores=rng.random((K, R), dtype=np.float32))

    target_rel = np.zeros((G, G, R), np.float32)
    for (s, o, p) in rels:
        target_rel[s, o, p] = 1.0
    target = dict(class_labels=torch.tensor(gt_cls, dtype=torch.int64),
                  boxes=torch.tensor([_cxcywh(b) for b in gt_boxes], dtype=torch.float32),
                  rel=torch.from_numpy(target_rel), orig_size=torch.tensor([H_IMG, W_IMG]))
    return target, phr, prd


def vrd_eval_inputs(seed=83):
    """(targets, phrdet entries, preddet entries): one item per image; the entries are dicts of numpy arrays."""
    rng = _rng(seed)
    out = [_image(rng, i, K) for i, K in enumerate(KS_OF_IMAGE)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


# ---- images built by hand (not part of the fixture: their expected values are worked out in the comments) ----------------
def _hand_target(boxes, classes, rels, num_rel, size=64):
    """boxes: integer xyxy on a size x size image (multiples of 1/128 once normalised: exact in float32)."""
    G = len(boxes)
    rel = torch.zeros(G, G, num_rel)
    for s, o, p in rels:
        rel[s, o, p] = 1.0
    cxcywh = [[(x0 + x1) / 2 / size, (y0 + y1) / 2 / size, (x1 - x0) / size, (y1 - y0) / size] for x0, y0, x1, y1 in boxes]
    return dict(class_labels=torch.tensor(classes), boxes=torch.tensor(cxcywh, dtype=torch.float32), rel=rel,
                orig_size=torch.tensor([size, size]))


def phrdet_hand_image():
    """(candidate dict, target, expected phrdet first ranks, K).  GT triplets in gt_entry order:
      (0, 1, p0)  GT union [0,0,39,9]; candidate 0 has a subject with IoU 0.25 and the GT's object: its union [6,0,39,9]
                  has IoU 340/400 = 0.85 -- phrdet matches at rank 0, sgdet never does;
      (0, 2, p1)  GT union [0,0,9,9]; candidate 1's union is [0,0,9,4]: intersection 50, union 100 under the +1
                  convention -- IoU exactly 0.5, a match (>=) at rank 1;
      (0, 2, p2)  same GT union; candidate 2's union is [0,0,6,6]: 49 / 100 = 0.49, labels agree, no match (rank K = 3)."""
    target = _hand_target([(0, 0, 9, 9), (30, 0, 39, 9), (2, 2, 5, 5)], [1, 2, 3], [(0, 1, 0), (0, 2, 1), (0, 2, 2)], 4)
    cand = dict(pred_boxes=torch.tensor([[6, 0, 15, 9], [30, 0, 39, 9], [0, 0, 9, 4], [2, 2, 5, 4], [0, 0, 6, 6],
                                         [2, 2, 5, 5]], dtype=torch.float32),
                pred_classes=torch.tensor([1, 2, 1, 3, 1, 3]),
                pred_rel_inds=torch.tensor([[0, 1, 0], [2, 3, 1], [4, 5, 2]]),
                rel_scores=torch.tensor([0.9, 0.8, 0.7]))
    return cand, target, [0, 1, 3], 3


def preddet_hand_image():
    """(candidate dict, target, expected chosen rows, first ranks, per-predicate first ranks) with R = 4, None = no entry
    equals the triplet.  GT rows j (gt_entry order) and the candidate rows they choose:
      j0 (0, 1, p0) -> row 1;  j1 (0, 1, p2) -> row 1 (a GT pair with two predicates);  j2 (1, 2, p0) -> row 0;
      j3 (2, 3, p1) -> no candidate has (2, 3): row 0, whose pair (1, 2) is j2's.  Row 3 repeats (0, 1) and is never chosen.
    Entries by flat index j * 4 + p:  j0 .5 .3 .9 .6 | j1 .5 .3 .9 .6 | j2 .5 .7 .1 .2 | j3 .5 .7 .1 .2.  Descending
    score, ties by ascending flat index:  .9 (2) .9 (6) .7 (9) .7 (13) .6 (3) .6 (7) .5 (0) .5 (4) .5 (8) .5 (12) ...
      j0: entries with pair (0, 1) and p0 are flat 0 and 4 -> first rank 6;  j1: flat 2 and 6 -> 0;
      j2: pair (1, 2), p0: flat 8 and 12 -> 8 (an order that put flat 8 ahead of flat 0 or 4 would say 6 or 7);
      j3: no entry carries (2, 3) -> none.
    Inside the rows of one predicate -- p0: j0, j2 -> .9 .7 .6 .5 (j0) .5 (j2): j0 at 3, j2 at 4;  p2: j1 alone -> 0."""
    target = _hand_target([(0, 0, 9, 9), (10, 0, 19, 9), (20, 0, 29, 9), (30, 0, 39, 9)], [1, 2, 3, 4],
                          [(0, 1, 0), (0, 1, 2), (1, 2, 0), (2, 3, 1)], 4)
    cand = dict(pred_rel_inds=torch.tensor([[1, 2], [0, 1], [3, 0], [0, 1]]),
                rel_scores=torch.tensor([[.5, .7, .1, .2], [.5, .3, .9, .6], [.8, .8, .8, .8], [1., 1., 1., 1.]]))
    return cand, target, [1, 1, 0, 0], [6, 0, 8, None], [3, 0, 4, None]
