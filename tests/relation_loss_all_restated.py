"""Helper (no tests): the UN-SAMPLED relation loss of csrc/loss.hip (rel_loss_all: evaluation mode, and training with both
``rel_sample_*`` None) restated in float64 numpy, three wrong neighbours of it, and the inputs of its tests -- shared by
tests/test_relation_loss_all_cpu.py (restatement pinned to the criterion's own composition, teeth of the neighbours) and
tests/test_gpu_relation_loss_all.py, so that both see identical inputs.

Definition, per image b:  tq[q] = target row of query q (matched: the matcher's pair; unmatched queries in ascending order
take rows T, T + 1, ...; an image the matcher refused -- index -1 -- has T = 0), wq[q] = 1 - sigmoid(matching cost of q, or
the non-matching cost),
    y(qa, qb, r) = t(tq[qa], tq[qb], r) * (wq[qa] * wq[qb])
    loss_rel     = sum bce_logits(x, y) / (B N N R),         bce_logits(x, y) = max(x, 0) - x y + log1p(exp(-|x|))
    grad_rel     = (sigmoid(x) - y) / (B N N R),             sigmoid(x) = 1 / (1 + exp(-x))
    loss_conn    = mean bce_logits(pred_conn, any_r t(tq[qa], tq[qb], r) != 0), grad_conn likewise over B N N.
The two expressions are the kernel's own, evaluated in float64: they fix what a +-inf logit gives (the reference's BCE differs
there)."""
import functools

import numpy as np
import torch

import loss_restated as LR

NM_COST = LR.NM_COST
NEIGHBOURS = ("no_weights", "identity_map", "unmatched_as_matched")
LOSS_BAR = 1e-5                      # relative; the bar of the training kernel (tests/test_gpu_loss_selection.py)


def grad_bar(count):
    """8 fp32 roundings of a value of magnitude <= 1, times the reciprocal of the element count"""
    return 8.0 * 2.0 ** -24 / count


def _sig(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z))


def _bce(x, y):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))


def maps(N, pred_idx, tgt_idx, cost, neighbour=None, nm_cost=NM_COST):
    """(tq [N] int64, wq [N] float64) of one image"""
    pi, ti = np.asarray(pred_idx, dtype=np.int64), np.asarray(tgt_idx, dtype=np.int64)
    cost = np.asarray(cost, dtype=np.float64)
    if len(pi) and (pi.min() < 0 or ti.min() < 0):       # refused by the matcher: an image without matches
        pi, ti, cost = pi[:0], ti[:0], cost[:0]
    T = len(pi)
    m = np.zeros(N, dtype=bool)
    m[pi] = True
    tq = np.zeros(N, dtype=np.int64)
    tq[pi] = ti
    tq[~m] = T + np.arange(N - T)
    c = np.full(N, float(nm_cost))
    c[pi] = cost
    if neighbour == "identity_map":
        tq = np.arange(N, dtype=np.int64)
    elif neighbour == "unmatched_as_matched":
        c[~m] = 0.0 if float(nm_cost) != 0.0 else 2.0    # a cost the matcher could have returned: w = 1 / 2 (or 0.12)
    wq = 1.0 - _sig(c)
    if neighbour == "no_weights":
        wq = np.ones(N)
    return tq, wq


def restate(pred_rel, pred_conn, dense, indices, costs, nm_cost=NM_COST, neighbour=None):
    """float64: (loss_rel, loss_conn, grad_rel [B, N, N, R], grad_conn [B, N, N, 1]).  ``dense``: per image the [N, N, R] target
    in TARGET order (build it from triplets with loss_restated.dense_of)."""
    assert neighbour in (None,) + NEIGHBOURS
    x = pred_rel.double().numpy()
    xc = pred_conn.double().numpy()
    B, N, _, R = x.shape
    y, yc = np.zeros_like(x), np.zeros_like(xc)
    for b in range(B):
        tq, wq = maps(N, indices[b][0].numpy(), indices[b][1].numpy(), costs[b].numpy(), neighbour, nm_cost)
        t = dense[b].double().numpy()[tq][:, tq]
        y[b] = t * (wq[:, None] * wq[None, :])[:, :, None]
        yc[b] = (t != 0).any(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        loss_rel = float(_bce(x, y).sum() / x.size)
        loss_conn = float(_bce(xc, yc).sum() / xc.size)
    return loss_rel, loss_conn, (_sig(x) - y) / x.size, (_sig(xc) - yc) / xc.size


# ------------------------------------------------------------------------------------------------------------------ cases
PLANTS = (0.0, -0.0, 88.0, -88.0, 1e4, -1e4, 1e-40)     # 1e-40: a denormal
NONFINITE = (float("inf"), float("-inf"), float("nan"))
COST_PLANTS = (-40.0, 40.0, 0.0)                          # both sigmoid tails (w = 1, w = 0) and the middle (w = 1 / 2)
# ... of the first matched queries of every image; where an image has few matches and w = 0 would silence all of its pairs:
_COST_PLANTS = {("n5r4", 0): (-40.0, 0.0), ("n5r4", 1): (40.0,), ("n6r65", 0): (0.0, -40.0)}


def cost_plants(name, b):
    return _COST_PLANTS.get((name, b), COST_PLANTS)

#       name          B  N     R   matched queries per image (as a matcher may order them)
CASES = {
    "n3r1":      (1, 3, 1, [[]]),                                              # no match, no relation
    "n5r4":      (2, 5, 4, [[3, 0, 4, 1, 2], [2]]),                           # all matched, non-monotonic | one match, no relation
    "n9r50":     (3, 9, 50, [[7, 2, 8, 0], [], [4, 8, 1, 0, 6, 3, 7, 2, 5]]),  # N R = 450: no multiple of 256 or of 4
    "n7r64":     (1, 7, 64, [[5, 0, 3]]),                                      # bit 63 of some word set
    "n6r65":     (1, 6, 65, [[4, 1]]),                                         # dense entry only
    "n1030r1":   (1, 1030, 1, [[1026, 5]]),                                    # the scan of the maps runs twice (N > 1024)
}
NO_RELATION = {"n3r1": (0,), "n5r4": (1,)}               # images without a relation
# Which neighbours CAN move a tenth of a case's elements -- arithmetic, not a choice:
#   "n3r1" has no relation: y = 0 whatever the maps and the weights are, all three neighbours coincide with the definition;
#   in "n5r4" the only image with relations has no unmatched query, so their weight cannot matter there;
#   under the criterion's constant an unmatched query weighs 1 - sigmoid(NM_COST) = 4e-13 (0 in fp32), so y != 0 only between
#   MATCHED queries: a wrong map shows in y only where many queries are matched ("n5r4" image 0, "n9r50" image 2), not with 2
#   or 3 matches of which one weighs 0 (cost +40).
# So every case runs a second time with a non-matching cost of 0 (NM_HALF: an unmatched query weighs 1 / 2; the constant is an
# argument of the entries): there the rows T, T + 1, ... that unmatched queries take show in y, and the map and the unmatched
# weight have teeth in the small cases too.
NM_HALF = 0.0
TEETH = {NM_COST: {"n3r1": (), "n5r4": ("no_weights", "identity_map"), "n9r50": NEIGHBOURS,
                   "n7r64": ("no_weights", "unmatched_as_matched"), "n6r65": ("no_weights", "unmatched_as_matched"),
                   "n1030r1": ("no_weights", "unmatched_as_matched")},
         NM_HALF: {"n3r1": (), "n5r4": ("no_weights", "identity_map"), "n9r50": NEIGHBOURS, "n7r64": NEIGHBOURS,
                   "n6r65": NEIGHBOURS, "n1030r1": NEIGHBOURS}}
SPARSE_TRIPLETS = 20     # per image, as in the benchmark: most (subject, object) pairs carry no relation


@functools.lru_cache(maxsize=None)
def case(name, logits="finite", nonbinary=False, sparse=False):
    """A case as loss_restated.build_case gives it (pred_rel, pred_conn, trips, dense, indices, costs).  Targets: ~30 % of all
    (row, col, predicate) set, over ALL rows (also the rows unmatched queries take), so that a tenth of the elements feel every
    neighbour -- at R >= 50 every pair then carries some relation and the connectivity target is all ones, so ``sparse`` draws
    SPARSE_TRIPLETS triplets per image instead: there the connectivity sees a wrong pair flag or a wrong map.
    ``logits``: "finite" -- normal draws + PLANTS; "nonfinite" -- NONFINITE planted too.  ``nonbinary``: dense only,
    some ones become 0.5, and 2.0 where y stays <= 1 (a pair of the query whose cost is 0: w = 1 / 2)."""
    B, N, R, matched = CASES[name]
    rng = np.random.default_rng(5100 + sorted(CASES).index(name))
    x = rng.standard_normal((B, N, N, R)).astype(np.float32)
    images = []
    for b, pred in enumerate(matched):
        T = len(pred)
        t = rng.random((N, N, R)) < 0.3
        if sparse:
            t[:] = False
            t.reshape(-1)[rng.choice(t.size, SPARSE_TRIPLETS, replace=False)] = True
        if b in NO_RELATION.get(name, ()):
            t[:] = False
        if R == 64:
            t[1, 2, 63] = t[6, 6, 63] = True
        images.append((np.array(pred, dtype=np.int64), rng.permutation(T), np.argwhere(t)))
    c = LR.build_case(rng, x, images)
    for b, pred in enumerate(matched):                   # costs: the plants first, normal draws after them
        plant = cost_plants(name, b)[:len(pred)]
        c["costs"][b][:len(plant)] = torch.tensor(plant)
    if name == "n1030r1":                                 # identity pairs would hide a wrong map; these are not
        assert [int(v) for v in c["indices"][0][0]] == [1026, 5]
        c["indices"][0] = (c["indices"][0][0], torch.tensor([1, 0]))
    # Logits as a trained head gives them -- higher where the target is set (x = draw + 2 y): with logits independent of the
    # targets a change of y moves the loss by -sum x dy, a sum of random signs.  Then the planted values: +1e4 and -88 on
    # elements whose y lies inside (0, 1) where there are any (they feel dropped weights, and a wrong map where two weights are
    # inside (0, 1); preferably where the target read through an identity map is 0), -1e4 and +88 on set targets of an
    # unmatched query (they feel its weight); everything else anywhere.
    ys, inner, outer = [], [], []
    for b in range(B):
        tq, wq = maps(N, c["indices"][b][0].numpy(), c["indices"][b][1].numpy(), c["costs"][b].numpy())
        m = np.zeros(N, dtype=bool)
        m[c["indices"][b][0].numpy()] = True
        t = c["dense"][b].numpy()[tq][:, tq]
        ww = (wq[:, None] * wq[None, :])[:, :, None]
        ys.append(t * ww)
        un = ~(m[:, None] & m[None, :])[:, :, None]
        wo = np.where(m, wq, 1.0)
        pool = (t != 0) & (ww <= 0.99) & ((ww >= 0.01) | ~(ww >= 0.01).any())
        felt = pool & (c["dense"][b].numpy() == 0)       # ... and where an identity map would read a 0 target, if anywhere
        inner.append(felt if felt.any() else pool)
        outer.append((t != 0) & un & ((wo[:, None] * wo[None, :])[:, :, None] >= 0.25))
    x = (x + 2.0 * np.stack(ys)).astype(np.float32)
    plants = (NONFINITE if logits == "nonfinite" else ()) + PLANTS
    plants = plants[:x.size]
    free = np.ones(x.size, dtype=bool)
    pools = {1e4: np.stack(inner), -88.0: np.stack(inner), -1e4: np.stack(outer), 88.0: np.stack(outer)}
    for v in plants:
        pool = np.nonzero(free & pools[v].reshape(-1))[0] if v in pools else []
        pool = pool if len(pool) else np.nonzero(free)[0]
        at = int(rng.choice(pool))
        x.reshape(-1)[at], free[at] = np.float32(v), False
    c["pred_rel"] = torch.as_tensor(x)
    if nonbinary:
        assert name == "n9r50"
        d = c["dense"][0]
        ones = d.nonzero()
        d[tuple(ones[::7].T)] = 0.5
        row = int(c["indices"][0][1][2])                 # the target row of the query with cost 0
        assert float(c["costs"][0][2]) == 0.0
        d[row, :, ::3] = torch.where(d[row, :, ::3] != 0, torch.tensor(2.0), torch.tensor(0.0))
        c["trips"] = None
    return c


def case_names(packed=None):
    return [n for n in CASES if packed is None or (CASES[n][2] <= 64) == packed]


# ------------------------------------------------------------------------------------------------- shared by the test files
def criterion(N, R, model_training):
    """The criterion on the un-sampled route: evaluation mode, or training mode with both sample counts None."""
    import types

    from egtr_amd.egtr import SceneGraphGenerationLoss
    matcher = types.SimpleNamespace(class_cost=2.0, bbox_cost=5.0, giou_cost=2.0)
    return SceneGraphGenerationLoss(matcher=matcher, num_object_queries=N, num_classes=12, num_rel_labels=R, eos_coef=0.1,
                                    losses=["relations"], smoothing=1e-14,
                                    rel_sample_negatives=None if model_training else 80,
                                    rel_sample_nonmatching=None if model_training else 80, model_training=model_training,
                                    focal_alpha=0.25, rel_sample_negatives_largest=True, rel_sample_nonmatching_largest=True)


def matcher_flat(indices, costs, dev):
    """The matcher's packed outputs on ``dev``: (pred_idx, tgt_idx, match_cost, out_offsets)"""
    offs = [0]
    for a, _ in indices:
        offs.append(offs[-1] + int(a.shape[0]))
    pi = torch.cat([a for a, _ in indices]).to(dev)
    ti = torch.cat([b for _, b in indices]).to(dev)
    mc = torch.cat(list(costs)).float().to(dev)
    if pi.numel() == 0:          # keep the kernels' pointers valid
        pi, ti = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        mc = torch.zeros(1, device=dev)
    return pi, ti, mc, torch.tensor(offs, dtype=torch.int32).to(dev)
