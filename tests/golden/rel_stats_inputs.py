"""Seeded inputs of the relation-statistics / zero-shot recall fixture (tests/golden/rel_stats.npz,
make_golden_rel_stats.py), in the pattern of sgg_eval_inputs.py.

``train_split``: a synthetic training set of ``N_TRAIN`` images over ``C`` object classes and ``R`` predicates -- 0 to 9 objects and
0 to 12 relation rows per image, classes and predicates drawn from skewed distributions (so that many (class, class, predicate)
cells stay empty), rows duplicated now and then, image 3 without a relation and image 5 without an object.
``test_split``: ``N_TEST`` images with candidates for both evaluator modes, built like sgg_eval_inputs._image: GT objects with
integer pixel boxes on a 1024 x 512 image (normalised cxcywh that are exact binary fractions), per GT object an exact-copy
predicted object, a copy shifted to IoU exactly 0.5 (a match), one just below it and a wrong-class copy, then decoys of class
C - 1 (never a GT class); S planted slots of which the first K_CAND are the candidates; each GT triplet gets an exact-copy
candidate at a rank drawn from [0, 20), [20, 50), [50, 100), [100, S) (cut off) or none, plus decoys.  Every third image
draws its GT triplets from the cells the training set HAS (no zero-shot triplet), the others draw them freely.  The two modes
get independent placements."""
import numpy as np
import torch

H_IMG, W_IMG = 512, 1024
C, R = 7, 5            # num_labels, num_rel_labels
N_TRAIN, N_TEST = 40, 12
N = 64                 # predicted objects
S = 120                # planted slots
K_CAND = 100           # candidates per image
SEED = 3


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


_CLASS_P = np.array([0.3, 0.25, 0.2, 0.1, 0.07, 0.05, 0.03])
_PRED_P = np.array([0.4, 0.3, 0.15, 0.1, 0.05])


def train_split(seed=SEED):
    """[(classes int64 [n], rows int64 [K, 3])] as numpy arrays; rows (subject index, object index, zero-based predicate)."""
    rng = _rng(seed)
    out = []
    for i in range(N_TRAIN):
        n = 0 if i == 5 else int(rng.integers(1 if i == 3 else 0, 10))
        classes = rng.choice(C, n, p=_CLASS_P).astype(np.int64)
        K = 0 if (i == 3 or n < 2) else int(rng.integers(0, 13))
        rows = []
        while len(rows) < K:
            if rows and rng.random() < 0.25:
                rows.append(rows[int(rng.integers(0, len(rows)))])      # a duplicated row
                continue
            s, o = (int(v) for v in rng.choice(n, 2, replace=False))
            rows.append((s, o, int(rng.choice(R, p=_PRED_P))))
        out.append((classes, np.array(rows, np.int64).reshape(-1, 3)))
    return out


def train_targets(seed=SEED):
    """The training split as target dicts (class_labels, rel_triplets)."""
    return [{"class_labels": torch.from_numpy(c), "rel_triplets": torch.from_numpy(r)} for c, r in train_split(seed)]


def count(split):
    """counts[class[s], class[o], p] += 1 per row: int64 [C + 1, C + 1, R] (the generator checks it against the reference)."""
    m = np.zeros((C + 1, C + 1, R), np.int64)
    for classes, rows in split:
        for s, o, p in rows:
            m[classes[s], classes[o], p] += 1
    return m


def _cxcywh(box):
    x0, y0, x1, y1 = box
    return [(x0 + x1) / 2 / W_IMG, (y0 + y1) / 2 / H_IMG, (x1 - x0) / W_IMG, (y1 - y0) / H_IMG]


def _place(rng, rels, copy, half, below, wrong):
    """S slots (s, o, p) in rank order for one mode."""
    slots, free = [None] * S, list(range(S))

    def place(lo, hi, trip):
        cand = [r for r in free if lo <= r < hi]
        if not cand or trip in slots:
            return
        r = int(rng.choice(cand))
        free.remove(r)
        slots[r] = trip

    for (s, o, p) in rels:
        lo, hi = [(0, 20), (20, 50), (50, 100), (100, S), (0, 0)][int(rng.integers(0, 5))]
        place(lo, hi, (copy[s], copy[o], p))
        for _ in range(int(rng.integers(0, 3))):
            kind = int(rng.integers(0, 5))
            place(0, S, [(wrong[s], copy[o], p), (copy[s], wrong[o], p), (copy[s], copy[o], (p + 1) % R),
                         (half[s], copy[o], p), (below[s], copy[o], p)][kind])
    decoys = list(range(4 * len(copy), N))
    used = {(t[0], t[1]) for t in slots if t is not None}
    for r in free:   # fillers: distinct decoy pairs, never a match
        while True:
            s, o = (int(v) for v in rng.choice(decoys, 2, replace=False))
            if (s, o) not in used:
                break
        used.add((s, o))
        slots[r] = (s, o, int(rng.integers(0, R)))
    return slots


def _image(rng, seen, seen_only):
    G = int(rng.integers(4, 9))
    gt_boxes, gt_cls = [], []
    for _ in range(G):
        d = int(rng.integers(10, 50))
        a, b = 3 * d, int(rng.integers(20, 150))
        x0, y0 = int(rng.integers(0, W_IMG - a - 80)), int(rng.integers(0, H_IMG - b - 2))
        gt_boxes.append((x0, y0, x0 + a - 1, y0 + b - 1))
        gt_cls.append(int(rng.choice(C - 1, p=_CLASS_P[:C - 1] / _CLASS_P[:C - 1].sum())))
    cells = [(s, o, p) for s in range(G) for o in range(G) if s != o for p in range(R)]
    if seen_only:
        cells = [c for c in cells if seen[gt_cls[c[0]], gt_cls[c[1]], c[2]]]
    T = min(int(rng.integers(3, 11)), len(cells))
    rels = sorted(cells[i] for i in rng.choice(len(cells), T, replace=False))

    objs = []

    def add(cls, box):
        objs.append((cls, box))
        return len(objs) - 1

    copy, half, below, wrong = {}, {}, {}, {}
    for g, (box, cls) in enumerate(zip(gt_boxes, gt_cls)):
        x0, y0, x1, y1 = box
        d = (x1 - x0 + 1) // 3
        copy[g] = add(cls, box)
        half[g] = add(cls, (x0 + d, y0, x1 + d, y1))
        below[g] = add(cls, (x0 + d + 1, y0, x1 + d + 1, y1))
        wrong[g] = add((cls + 1) % (C - 1), box)
    while len(objs) < N:
        x0, y0 = int(rng.integers(0, W_IMG - 40)), int(rng.integers(0, H_IMG - 40))
        add(C - 1, (x0, y0, x0 + 30, y0 + 30))

    cand = {"pred_boxes": torch.tensor([b for _, b in objs], dtype=torch.float32),
            "pred_classes": torch.tensor([c for c, _ in objs], dtype=torch.int64)}
    for mode in ("m", "s"):
        slots = np.array(_place(rng, rels, copy, half, below, wrong)[:K_CAND], np.int64)
        top = (0.9 * (1 - 0.002 * np.arange(K_CAND))).astype(np.float32)
        if mode == "m":
            cand["m_inds"], cand["m_scores"] = torch.from_numpy(slots), torch.from_numpy(top)
        else:
            scores = rng.uniform(0, 0.3, (K_CAND, R)).astype(np.float32)
            scores[np.arange(K_CAND), slots[:, 2]] = top
            cand["s_inds"], cand["s_scores"] = torch.from_numpy(slots[:, :2].copy()), torch.from_numpy(scores)
    target = {"class_labels": torch.tensor(gt_cls, dtype=torch.int64),
              "boxes": torch.tensor([_cxcywh(b) for b in gt_boxes], dtype=torch.float32),
              "rel_triplets": torch.tensor(rels, dtype=torch.int64).reshape(-1, 3),
              "orig_size": torch.tensor([H_IMG, W_IMG])}
    return cand, target, np.array(gt_boxes, np.float32)


def test_split(seed=SEED):
    """(candidates, targets, gt_boxes): per image a dict (pred_boxes [N, 4] xyxy pixels, pred_classes [N], m_inds [K, 3],
    m_scores [K], s_inds [K, 2], s_scores [K, R]), the target dict (class_labels, boxes, rel_triplets in lexicographic
    order, orig_size) and the GT boxes in pixels (float32 [G, 4])."""
    seen = count(train_split(seed)) > 0
    rng = _rng(seed + 1000)
    out = [_image(rng, seen, seen_only=(i % 3 == 0)) for i in range(N_TEST)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


test_split.__test__ = False   # not a test, whatever collects this module


def candidates(cands, mode, device=None, top=None):
    """The evaluator's candidate dicts of one mode ("m": multiple predicates, "s": single), optionally the first ``top``."""
    out = []
    for c in cands:
        d = {"pred_boxes": c["pred_boxes"], "pred_classes": c["pred_classes"], "pred_rel_inds": c[f"{mode}_inds"][:top]}
        if mode == "s":
            d["rel_scores"] = c["s_scores"][:top]
        out.append({k: v.to(device) for k, v in d.items()} if device is not None else d)
    return out
