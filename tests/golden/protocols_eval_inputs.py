"""Seeded inputs of the PredCls / SGCls fixture (tests/golden/protocols_eval.npz, make_golden_protocols.py).

Model outputs (logits, pred_boxes, pred_rel, pred_connectivity) for N = 16 queries, targets in the reference's format
and, per image, the explicit GT object -> query mapping ``query_of`` (a random injection; no matcher is involved):
  * G per image runs over 2, 3, 7, 12, 16; the G = 2 images have 2 * 1 * R = 12 < 20 entries, fewer than the smallest k;
  * every GT relation gets a planted relation score at (query of s, query of o, p) from one of four bands (near 1,
    0.90 .. 0.96, 0.80 .. 0.90, below 0.3) among a background that is uniform in [0.05, 0.95), so the ranks of the exact
    candidates spread over the first 20, 50, 100 and beyond as the domain grows with G.  All values lie strictly inside
    (0, 1) and connectivity in [0.85, 1): every score of the domain is positive and (the generator asserts it) no two are
    equal;
  * the ``DUP`` images hold two GT objects of ONE class whose boxes differ by one pixel (IoU > 0.9), related to the same
    object by the same predicate where only ONE of the two relations is in the GT, and the planted score sits on the
    OTHER object's query: the candidate on the "wrong" GT object matches, as the reference's box test allows;
  * the logits give the matched query the GT class except for every third GT object, whose query predicts another class
    (SGCls loses the triplets on it); object scores differ between queries, so the SGCls order differs from PredCls;
  * the last predicate never occurs in the GT (the NaN path of the mean recall).
Boxes are integer pixels on a 1024 x 512 image, stored as normalised cxcywh that are exact binary fractions."""
import numpy as np
import torch

from sgg_eval_inputs import H_IMG, W_IMG, _cxcywh, _rng

N = 16                  # queries
R = 6                   # predicates; the last one never occurs in the GT
R_USED = R - 1
NUM_LABELS = 5
GS = (2, 3, 7, 12, 16, 7, 12, 2)
DUP = (2, 5)            # images whose GT objects 0 and 1 are near-copies of one class
BANDS = ((0.97, 0.999), (0.90, 0.96), (0.80, 0.90), (0.05, 0.30))


def _image(rng, i, G):
    gt_boxes, gt_cls = [], []
    for _ in range(G):
        a, b = int(rng.integers(30, 150)), int(rng.integers(20, 150))
        x0, y0 = int(rng.integers(0, W_IMG - a - 4)), int(rng.integers(0, H_IMG - b - 2))
        gt_boxes.append((x0, y0, x0 + a - 1, y0 + b - 1))
        gt_cls.append(int(rng.integers(0, NUM_LABELS)))
    dup = i in DUP
    if dup:
        x0, y0, x1, y1 = gt_boxes[0]
        gt_boxes[1] = (x0 + 1, y0, x1 + 1, y1)
        gt_cls[1] = gt_cls[0]
    query_of = rng.permutation(N)[:G].astype(np.int32)

    pairs = [(s, o) for s in range(G) for o in range(G) if s != o]
    if dup:
        pairs = [pr for pr in pairs if pr not in ((1, 2), (0, 1), (1, 0))]
    T = min(len(pairs), int(rng.integers(3, 10)))
    chosen = [pairs[j] for j in rng.choice(len(pairs), T, replace=False)]
    if dup and (0, 2) not in chosen:
        chosen[0] = (0, 2)
    rels = sorted((s, o, int(rng.integers(0, R_USED))) for s, o in chosen)

    rel = rng.uniform(0.05, 0.95, (N, N, R)).astype(np.float32)
    conn = rng.uniform(0.85, 1.0, (N, N, 1)).astype(np.float32)
    for (s, o, p) in rels:
        lo, hi = BANDS[int(rng.integers(0, len(BANDS)))]
        if dup and (s, o) == (0, 2):      # the planted score goes to GT object 1, the near-copy of object 0
            rel[query_of[1], query_of[o], p] = np.float32(0.995)
            rel[query_of[0], query_of[o], p] = np.float32(0.06)
        else:
            rel[query_of[s], query_of[o], p] = np.float32(rng.uniform(lo, hi))

    logits = rng.normal(0.0, 0.3, (N, NUM_LABELS + 1)).astype(np.float32)
    logits[:, NUM_LABELS] -= 1.0
    for g in range(G):
        cls = gt_cls[g] if (g % 3 != 2 or (dup and g == 2)) else (gt_cls[g] + 1) % NUM_LABELS
        logits[query_of[g], cls] += np.float32(rng.uniform(2.0, 4.0))
    boxes = rng.uniform(0.2, 0.6, (N, 4)).astype(np.float32)      # the query boxes: not read by these protocols

    target_rel = np.zeros((G, G, R), np.float32)
    for (s, o, p) in rels:
        target_rel[s, o, p] = 1.0
    target = dict(class_labels=torch.tensor(gt_cls, dtype=torch.int64),
                  boxes=torch.tensor([_cxcywh(b) for b in gt_boxes], dtype=torch.float32),
                  rel=torch.from_numpy(target_rel), orig_size=torch.tensor([H_IMG, W_IMG]))
    return logits, boxes, rel, conn, target, query_of


def protocols_eval_inputs(seed=97):
    """(outputs, targets, query_of): outputs dict of [B, ...] tensors, targets list of target dicts, query_of list of
    int32 arrays [G] (the query of every GT object)."""
    rng = _rng(seed)
    out = [_image(rng, i, G) for i, G in enumerate(GS)]
    stack = lambda j: torch.from_numpy(np.stack([o[j] for o in out]))  # noqa: E731
    outputs = {"logits": stack(0), "pred_boxes": stack(1), "pred_rel": stack(2), "pred_connectivity": stack(3)}
    return outputs, [o[4] for o in out], [o[5] for o in out]


class FixedMatcher:
    """A matcher that returns the fixture's mapping: what ``runtime.matched_triplet_candidates`` calls in place of the
    Hungarian matcher.  (pred_idx, tgt_idx) per image, in query order like the real one."""

    def __init__(self, query_of):
        self.query_of = query_of

    def __call__(self, outputs, targets):
        device = outputs["logits"].device
        out = []
        for q in self.query_of:
            q = torch.as_tensor(np.asarray(q), dtype=torch.int64)
            order = torch.argsort(q)
            out.append((q[order].to(device), order.to(device)))
        return out, None
