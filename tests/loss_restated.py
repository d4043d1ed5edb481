"""Helper (no tests): the training criterion of csrc/loss.hip restated in float64 numpy / torch-CPU, and the inputs of the
criterion's edge tests -- shared by tests/test_loss_cases_cpu.py (restatement pinned to the oracle, preconditions of every
case), tests/test_gpu_loss_selection.py, tests/test_gpu_detection_loss_edges.py and tests/test_gpu_deterministic.py, so that
the CPU tests and the GPU tests see identical inputs.

Geometry of the relation loss's final pass (rel_loss_final): one workgroup per query row ``qa``; the row's N R logits are
walked in STEPS of 256 consecutive indices e = qb R + r, a step is four WAVES of 64 lanes.  ``position(flat, N, R)`` names
these coordinates for a flat index (qa N + qb) R + r."""
import functools
import types

import numpy as np
import torch

from oracle import loss as OL

STEP, WAVE = 256, 64      # kLT of loss.hip, the wave size of gfx950
NM_COST = float(OL.nonmatching_cost(2.0, 5.0, 2.0, 1e-14))


# ---------------------------------------------------------------------------------------------------------- selection
def key_of(x):
    """loss.hip key_of(): the order-preserving uint32 image of an fp32 value (larger float <-> larger key; -0.0 maps just
    below +0.0)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _rank(flat, order):
    """What "larger" means: "value" -- float comparison (-0.0 == +0.0); "key" -- key_of()."""
    if order == "value":
        return flat.astype(np.float64)
    if order == "key":
        return key_of(flat).astype(np.int64)
    raise ValueError(order)


def topk_lowest_index_first(logits, candidates, k, order="value"):
    """Boolean mask (shape of ``logits``) of the ``k`` candidates with the largest logit, ties broken by the LOWEST flat
    (C-order) index: top-k by (logit descending, flat index ascending)."""
    flat, cand = np.asarray(logits).reshape(-1), np.asarray(candidates).reshape(-1)
    idx = np.nonzero(cand)[0]
    order_idx = idx[np.lexsort((idx, -_rank(flat[idx], order)))]   # last key is the primary one
    sel = np.zeros(flat.shape, dtype=bool)
    sel[order_idx[:k]] = True
    return sel.reshape(np.asarray(logits).shape)


def _select(pred_rel, dense, pred_idx, tgt_idx, k_neg, k_nm, order):
    N, _, R = pred_rel.shape
    pred_idx, tgt_idx = np.asarray(pred_idx, dtype=np.int64), np.asarray(tgt_idx, dtype=np.int64)
    T = len(pred_idx)
    matched = np.zeros(N, dtype=bool)
    matched[pred_idx] = True
    tq = np.zeros(N, dtype=np.int64)
    tq[pred_idx] = tgt_idx
    tq[~matched] = T + np.arange(N - T)          # unmatched queries in ascending order take rows T, T + 1, ...
    t = dense[tq][:, tq]                          # target in query order
    blk = (matched[:, None] & matched[None, :])[:, :, None].repeat(R, 2)
    n_true, n_false = int((t[blk] != 0).sum()), int((t[blk] != 1).sum())
    n_nm = (N * N - T * T) * R
    k = (min(n_true * k_neg, n_false), min(n_true * k_nm, n_nm)) if n_true > 0 else (0, 0)
    rank = _rank(np.asarray(pred_rel).reshape(-1), order).reshape(pred_rel.shape)
    mult = (blk & (t != 0)).astype(np.int64)
    cands, sels, tieds, aboves, info = (blk & (t != 1), ~blk), [], [], [], []
    for prob, cand in enumerate(cands):
        sel = topk_lowest_index_first(pred_rel, cand, k[prob], order)
        mult += sel
        if k[prob]:
            thr = np.sort(rank[cand])[::-1][k[prob] - 1]
            tied, above = cand & (rank == thr), cand & (rank > thr)
            info.append((k[prob], int(tied.sum()), k[prob] - int(above.sum())))
        else:
            tied = above = np.zeros_like(cand)
            info.append((0, 0, 0))
        sels.append(sel)
        tieds.append(tied)
        aboves.append(above)
    return types.SimpleNamespace(mult=mult, t=t, matched=matched, info=info, cand=cands, sel=sels, tied=tieds, above=aboves,
                                 n_true=n_true)


def relation_selection(pred_rel, dense, pred_idx, tgt_idx, k_neg, k_nm, order="value"):
    """One image of the relation loss (model/egtr.py:754-923, largest-score sampling) in query order, with the deterministic
    tie rule.  pred_rel [N, N, R]; dense [N, N, R] targets in TARGET order; pred_idx / tgt_idx: the matcher's pairs.
    Returns (mult [N, N, R] int: how often an element enters the mean, target in query order, matched [N] bool,
    per problem (k, tied candidates at the threshold, of which needed))."""
    s = _select(pred_rel, dense, pred_idx, tgt_idx, k_neg, k_nm, order)
    return s.mult, s.t, s.matched, s.info


def position(flat, N, R):
    """(query row, step of the row, wave of the step) of a flat index of an image's [N, N, R] logits."""
    row, e = divmod(int(flat), N * R)
    return row, e // STEP, (e % STEP) // WAVE


def relation_expectation(case, k_neg, k_nm, order="key"):
    """float64 numpy, the whole batch: ``mult`` [B, N, N, R]; ``grad`` = mult (sigmoid(x) - y) / total; ``loss_rel``; ``info``
    per image and problem (k, tied, need); ``total``; ``unit`` = (sigmoid(x) - y) / total; ``images``: the per-image selection
    (candidate / selected / tied / above-threshold masks per problem); ``cuts`` per image and problem: position() of the LAST
    tied candidate that is taken, or None."""
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))  # noqa: E731
    N, R = case["N"], case["R"]
    mults, ys, images = [], [], []
    for b in range(case["B"]):
        pi, ti = case["indices"][b][0].numpy(), case["indices"][b][1].numpy()
        s = _select(case["pred_rel"][b].numpy(), case["dense"][b].numpy(), pi, ti, k_neg, k_nm, order)
        w = np.full(N, 1.0 - sig(NM_COST))
        w[pi] = 1.0 - sig(case["costs"][b].double().numpy())
        mults.append(s.mult)
        ys.append(s.t.astype(np.float64) * (w[:, None] * w[None, :])[:, :, None])
        images.append(s)
    mult, y, x = np.stack(mults), np.stack(ys), case["pred_rel"].double().numpy()
    total = int(mult.sum())
    bce = np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = (sig(x) - y) / total
        loss = float((mult * bce).sum() / total)
    cuts = []
    for s in images:
        taken = [np.nonzero((s.sel[p] & s.tied[p]).reshape(-1))[0] for p in range(2)]
        cuts.append([position(f[-1], N, R) if len(f) else None for f in taken])
    return types.SimpleNamespace(mult=mult, grad=mult * unit, loss_rel=loss, info=[s.info for s in images], total=total,
                                 unit=unit, images=images, cuts=cuts)


# --------------------------------------------------------------------------------------------------------- generators
def dense_of(trips, N, R):
    rel = torch.zeros(N, N, R)
    if len(trips):
        rel[trips[:, 0], trips[:, 1], trips[:, 2]] = 1.0
    return rel


def distinct_logits(rng, *shape):
    """fp32 logits in (-4, 4), no two equal: a random permutation of an evenly spaced grid."""
    n = int(np.prod(shape))
    assert n < 2 ** 24
    return (((rng.permutation(n).astype(np.float32) + 0.5) / n - 0.5) * 8.0).astype(np.float32).reshape(shape)


def three_valued(rng, *shape):
    return ((rng.integers(0, 3, shape) - 1) * 0.5).astype(np.float32)


def build_case(rng, pred_rel, images):
    """images: per image (pred_idx, tgt_idx, triplets [K, 3] in TARGET order).  Dense targets hold 1 at the triplets."""
    B, N, _, R = pred_rel.shape
    trips = [torch.as_tensor(np.asarray(t, dtype=np.int64).reshape(-1, 3)) for _, _, t in images]
    indices = [(torch.as_tensor(np.asarray(p, dtype=np.int64)), torch.as_tensor(np.asarray(t, dtype=np.int64)))
               for p, t, _ in images]
    costs = [torch.as_tensor((rng.standard_normal(len(p)) * 3).astype(np.float32)) for p, _, _ in images]
    pred_conn = torch.as_tensor(rng.standard_normal((B, N, N, 1)).astype(np.float32))
    return dict(B=B, N=N, R=R, pred_rel=torch.as_tensor(np.ascontiguousarray(pred_rel, dtype=np.float32)),
                pred_conn=pred_conn, trips=trips, dense=[dense_of(t, N, R) for t in trips], indices=indices, costs=costs)


def k_for_cut(case, prob, value, where, b=0):
    """The k for which the lowest-index-first selection of problem ``prob`` of image ``b`` ends AT the first candidate (flat
    order) whose logit equals ``value`` and whose position satisfies ``where(row, step, wave)``: every candidate above
    ``value`` plus the tied ones up to and including that one."""
    N, R = case["N"], case["R"]
    x = case["pred_rel"][b].numpy()
    s = _select(x, case["dense"][b].numpy(), case["indices"][b][0].numpy(), case["indices"][b][1].numpy(), 0, 0, "key")
    assert s.n_true == 1                              # then k[prob] is the sample count itself, up to the candidate count
    cand = s.cand[prob].reshape(-1)
    tied = np.nonzero(cand & (x.reshape(-1) == np.float32(value)))[0]
    hit = [i for i, f in enumerate(tied) if where(*position(f, N, R))]
    assert hit, "no tied candidate at such a position"
    return int((cand & (x.reshape(-1) > np.float32(value))).sum()) + hit[0] + 1


@functools.lru_cache(maxsize=None)
def steps_case():
    """B1: N R = 1200 -- four full steps and one of 176 lanes per row.  ``ks``: "mid" cuts in steps 2 (block) and 1 (outside),
    "last" cuts in the partial fifth step."""
    rng = np.random.default_rng(4101)
    N, R = 24, 50
    pred = np.array([1, 4, 7, 10, 13, 16, 19, 22])
    c = build_case(rng, three_valued(rng, 1, N, N, R), [(pred, rng.permutation(8), [[2, 5, 17]])])
    c["ks"] = {
        "mid": (k_for_cut(c, 0, 0.0, lambda row, step, wave: row >= 13 and step == 2 and wave >= 1),
                k_for_cut(c, 1, 0.0, lambda row, step, wave: row >= 11 and step == 1 and wave >= 2)),
        "last": (k_for_cut(c, 0, 0.0, lambda row, step, wave: row >= 16 and step == 4 and wave >= 1),
                 k_for_cut(c, 1, 0.0, lambda row, step, wave: row >= 9 and step == 4 and wave >= 2)),
    }
    return c


@functools.lru_cache(maxsize=None)
def rows_case():
    """B2: matched queries on both sides of 256; both cuts in a row >= 256 (the tie-count prefix loop of that row's
    workgroup runs twice for its low threads) and in a step >= 1."""
    rng = np.random.default_rng(4102)
    N, R = 264, 3
    pred = np.array([3, 40, 90, 130, 170, 200, 230, 250, 257, 259, 261, 263])
    c = build_case(rng, three_valued(rng, 1, N, N, R), [(pred, rng.permutation(12), [[7, 1, 2]])])
    c["ks"] = {"rows": (k_for_cut(c, 0, 0.0, lambda row, step, wave: row >= 259 and step >= 2 and wave >= 1),
                        k_for_cut(c, 1, 0.0, lambda row, step, wave: row >= 258 and step >= 1 and wave >= 1))}
    return c


SCAN_T = 12


@functools.lru_cache(maxsize=None)
def scan_case():
    """B3: N = 1030 > kPrepT = 1024.  Matched and unmatched queries on both sides of 1024; dense targets at rows / columns >= T
    (target rows of UNMATCHED queries, the last two beyond row 1024) whose logits lie above (sampled: 0.5) or below (never
    sampled: -0.5) the tied threshold 0; the cut of the outside-block problem in a row >= 1024."""
    rng = np.random.default_rng(4103)
    N, R, T = 1030, 1, SCAN_T
    pred = np.array([1026, 5, 300, 1024, 511, 100, 512, 700, 1029, 900, 1000, 1023])      # as a matcher may order them
    extra = [[1027, 3, 0], [2, 1029, 0], [400, 1028, 0], [1029, 1027, 0], [700, 20, 0], [1028, 5, 0]]   # rows / cols >= T
    x = three_valued(rng, 1, N, N, R)
    c = build_case(rng, x, [(pred, rng.permutation(T), [[4, 9, 0]] + extra)])
    tq = target_rows(c)
    q_of = {int(r): q for q, r in enumerate(tq)}
    for i, (a, o, _) in enumerate(extra):
        x[0, q_of[a], q_of[o], 0] = -0.5 if i == len(extra) - 1 else 0.5
    c["pred_rel"] = torch.as_tensor(x)
    c["extra"] = extra
    c["ks"] = {"scan": (k_for_cut(c, 0, 0.0, lambda row, step, wave: row >= 700),
                        k_for_cut(c, 1, 0.0, lambda row, step, wave: row >= 1025 and step >= 2))}
    return c


def target_rows(c, b=0):
    """query -> target row, as the reference permutes (matched rows first, unmatched queries ascending)."""
    N, (pi, ti) = c["N"], c["indices"][b]
    tq = np.zeros(N, dtype=np.int64)
    m = np.zeros(N, dtype=bool)
    m[pi.numpy()] = True
    tq[pi.numpy()] = ti.numpy()
    tq[~m] = len(pi) + np.arange(N - len(pi))
    return tq


RADIX_FAMILIES = ("one_bin", "one_bin_negative", "low_bits", "low_bits_negative", "powers", "zeros")
RADIX_KS = (1, 2, 37, 500, 10 ** 6)


@functools.lru_cache(maxsize=None)
def radix_case(family):
    """B4: N = 16, R = 8 (2048 logits), T = 6, one true relation; the logits built from bit patterns."""
    rng = np.random.default_rng(4200 + RADIX_FAMILIES.index(family))
    N, R, n = 16, 8, 16 * 16 * 8
    if family in ("one_bin", "one_bin_negative"):        # [1, 1.25): bits 30..21 shared, all distinct
        u = np.uint32(0x3F800000) + rng.choice(1 << 21, n, replace=False).astype(np.uint32)
    elif family in ("low_bits", "low_bits_negative"):    # 22 shared leading bits, 2048 draws of 1024 values
        u = np.uint32(0x3F800000) | rng.integers(0, 1024, n).astype(np.uint32)
    if family in ("one_bin", "low_bits"):
        x = u.view(np.float32)
    elif family in ("one_bin_negative", "low_bits_negative"):
        x = (u | np.uint32(0x80000000)).view(np.float32)
    elif family == "powers":
        x = (rng.choice([-1.0, 1.0], n) * np.exp2(rng.uniform(-100, 6, n))).astype(np.float32)
    else:
        # few values above the zeros: the thresholds of k = 37 and k = 500 fall on +0.0, among several hundred tied zeros
        x = rng.choice(np.array([-1.0, -2.0 ** -140, -0.0, 0.0, 2.0 ** -140, 1.0], dtype=np.float32), n,
                       p=[0.2, 0.2, 0.25, 0.25, 0.05, 0.05])
    pred = np.array([0, 3, 7, 8, 12, 15])
    return build_case(rng, np.ascontiguousarray(x, dtype=np.float32).reshape(1, N, N, R),
                      [(pred, rng.permutation(6), [[1, 4, 6]])])


@functools.lru_cache(maxsize=None)
def degenerate_case(distinct=False):
    """B5: image 0 all queries matched, image 1 without targets, image 2 targets without a relation, image 3 ordinary."""
    rng = np.random.default_rng(4300 + int(distinct))
    N, R = 9, 7
    x = distinct_logits(rng, 4, N, N, R) if distinct else three_valued(rng, 4, N, N, R)
    none = np.zeros((0, 3), dtype=np.int64)
    images = [(rng.permutation(N), rng.permutation(N), [[0, 5, 3], [8, 8, 6], [2, 1, 0]]),
              (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), none),
              (np.array([1, 4, 6]), rng.permutation(3), none),
              (np.array([0, 2, 3, 7, 8]), rng.permutation(5), [[1, 3, 2], [4, 0, 6]])]
    return build_case(rng, x, images)


def single_image(c, b):
    """Image ``b`` of a case as a batch of its own."""
    return dict(c, B=1, pred_rel=c["pred_rel"][b:b + 1].contiguous(), pred_conn=c["pred_conn"][b:b + 1].contiguous(),
                trips=c["trips"][b:b + 1], dense=c["dense"][b:b + 1], indices=c["indices"][b:b + 1],
                costs=c["costs"][b:b + 1])


@functools.lru_cache(maxsize=None)
def nonbinary_case():
    """B6: tie-free logits, dense targets with block entries 0.5 and 2.0 -- each counts as a true relation (!= 0) AND as a false
    candidate (!= 1) in the reference.  The second image is an ordinary 0 / 1 one.  No triplet form exists."""
    rng = np.random.default_rng(4400)
    N, R = 12, 5
    images = [(np.array([0, 2, 5, 6, 9, 11]), rng.permutation(6), [[1, 2, 3], [4, 4, 0]]),
              (np.array([3, 4, 10]), rng.permutation(3), [[0, 2, 1]])]
    c = build_case(rng, distinct_logits(rng, 2, N, N, R), images)
    c["dense"][0][3, 1, 2] = 0.5
    c["dense"][0][0, 5, 4] = 2.0
    c["dense"][0][2, 2, 1] = 0.5
    c["trips"] = None
    # the 0.5 / 2.0 elements must be reachable by the sampling: make two of them the largest logits of their image
    tq = target_rows(c)
    q_of = {int(r): q for q, r in enumerate(tq)}
    x = c["pred_rel"].numpy().copy()
    x[0, q_of[3], q_of[1], 2], x[0, q_of[0], q_of[5], 4] = 4.5, 4.25
    c["pred_rel"] = torch.as_tensor(x)
    return c


@functools.lru_cache(maxsize=None)
def plain_case():
    """Tie-free, 0 / 1 targets, B = 3 with an image without targets: pins the restatement to the oracle."""
    rng = np.random.default_rng(4500)
    N, R = 11, 6
    images = [(np.array([7, 1, 4, 10, 2]), rng.permutation(5), [[0, 1, 2], [3, 3, 5], [4, 0, 0]]),
              (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros((0, 3), dtype=np.int64)),
              (np.array([0, 5, 6, 9]), rng.permutation(4), [[2, 1, 4]])]
    return build_case(rng, distinct_logits(rng, 3, N, N, R), images)


def oracle_relation(case, k_neg, k_nm):
    """oracle.loss.relation_losses in float64 under autograd: (loss_rel, loss_connectivity, grad_rel, grad_conn)."""
    pr = case["pred_rel"].double().requires_grad_(True)
    pc = case["pred_conn"].double().requires_grad_(True)
    l_rel, l_conn = OL.relation_losses(pr, pc, [{"rel": d.double()} for d in case["dense"]], case["indices"],
                                       [x.double() for x in case["costs"]], NM_COST, k_neg, k_nm, True)
    g_rel, = torch.autograd.grad(l_rel, pr, retain_graph=True)
    g_conn, = torch.autograd.grad(l_conn, pc)
    return float(l_rel.detach()), float(l_conn.detach()), g_rel.numpy(), g_conn.numpy()


# ---------------------------------------------------------------------------------------------------- detection losses
def detection_expectation(logits, boxes, indices, targets, focal_alpha, num_boxes, weights):
    """oracle.loss.labels_boxes_card in float64 under autograd.  ``indices``: per image (pred_idx, tgt_idx); a target label
    outside [0, C) means "no object" (loss.hip, det_loss_f32).  Returns (losses as floats, d total / d logits, d total / d boxes,
    d loss_bbox / d boxes, d loss_giou / d boxes) with total = sum_k weights[k] losses[k]."""
    C = logits.shape[-1]
    lg = logits.double().requires_grad_(True)
    bx = boxes.double().requires_grad_(True)
    tg = []
    for t in targets:
        lab = t["class_labels"].clone()
        lab[(lab < 0) | (lab >= C)] = C
        tg.append({"class_labels": lab, "boxes": t["boxes"].double()})
    losses = OL.labels_boxes_card(lg, bx, indices, tg, num_boxes, focal_alpha)
    total = sum(losses[k] * w for k, w in weights.items())
    g_lg, g_bx = torch.autograd.grad(total, [lg, bx], retain_graph=True)
    g_l1, = torch.autograd.grad(losses["loss_bbox"], bx, retain_graph=True)
    g_giou, = torch.autograd.grad(losses["loss_giou"], bx)
    return {k: float(v) for k, v in losses.items()}, g_lg, g_bx, g_l1, g_giou
