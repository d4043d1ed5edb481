"""Shared by tests/test_protocols_eval_cpu.py and tests/test_gpu_protocols_eval.py: the matched top-K definition restated
as a brute-force Python sort (one float32 rounding per product, the whole domain sorted by (descending score key,
ascending (s, o, p))), seeded inputs for it, and a NaN-aware comparison of its outputs."""
import numpy as np
import torch


def score_key(x):
    """csrc/order_key.h: a larger key ranks earlier; NaN is the smallest key, -0 = +0."""
    x = np.float32(x)
    if np.isnan(x):
        return 0
    if x == 0:
        x = np.float32(0.0)
    u = int(np.array(x, np.float32).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def _clamp(x):
    x = np.float32(x)
    return x if np.isnan(x) else min(max(x, np.float32(0.0)), np.float32(1.0))


def brute_force(pred_rel, pred_conn, query_of, obj_score, K, mode):
    """(inds, rel_scores, triplet_scores, count) as ``ops.matched_topk`` defines them, by sorting every entry."""
    rel = pred_rel.numpy()
    conn = None if pred_conn is None else pred_conn.numpy().reshape(rel.shape[:3])
    qof, obj = query_of.numpy(), obj_score.numpy()
    B, N, _, R = rel.shape
    Gp = qof.shape[1]
    cols = 3 if mode == 0 else 2
    inds = np.full((B, K, cols), Gp - 1, np.int64)
    rel_scores = np.zeros((B, K) if mode == 0 else (B, K, R), np.float32)
    trip = np.zeros((B, K), np.float32)
    count = np.zeros(B, np.int32)
    for b in range(B):
        entries = []
        for s in range(Gp):
            for o in range(Gp):
                if s == o or not (0 <= qof[b, s] < N and 0 <= qof[b, o] < N):
                    continue
                so = np.float32(obj[b, s]) * np.float32(obj[b, o])
                row = [_clamp(v) for v in rel[b, qof[b, s], qof[b, o]]]
                if conn is not None:
                    c = _clamp(conn[b, qof[b, s], qof[b, o]])
                    row = [np.float32(v * c) for v in row]
                if mode == 0:
                    for p, r in enumerate(row):
                        score = np.float32(r * so)
                        entries.append((-score_key(score), s, o, p, r, score))
                else:
                    m = np.float32("nan") if any(np.isnan(v) for v in row) else max(row)
                    score = np.float32(m * so)
                    entries.append((-score_key(score), s, o, 0, row, score))
        entries.sort(key=lambda e: e[:4])
        n = min(K, len(entries))
        count[b] = n
        for k, (_, s, o, p, r, score) in enumerate(entries[:n]):
            inds[b, k] = (s, o, p)[:cols]
            rel_scores[b, k] = r
            trip[b, k] = score
    return tuple(torch.from_numpy(x) for x in (inds, rel_scores, trip, count))


def same(got, want):
    """Index-exact and value-exact (NaN equals NaN, -0 equals +0) on all four outputs."""
    for g, w in zip(got, want):
        g, w = g.cpu(), w.cpu()
        if g.shape != w.shape or g.dtype != w.dtype:
            return False
        if g.is_floating_point():
            if not torch.equal(g.isnan(), w.isnan()) or not torch.equal(g.nan_to_num(nan=-7.0), w.nan_to_num(nan=-7.0)):
                return False
        elif not torch.equal(g, w):
            return False
    return True


def random_inputs(seed, B, N, R, Gp, matched, quant=0, conn=True):
    """pred_rel in [-0.2, 1.2) (the clamp bites), pred_conn in [-0.1, 1.1), obj_score in [0.3, 1); ``matched[b]`` GT
    objects of image b (random ones among the Gp) get distinct random queries.  ``quant`` > 0 rounds every value to
    multiples of 1 / quant: few distinct scores, many ties."""
    rng = np.random.Generator(np.random.PCG64(seed))
    q = (lambda x: np.round(x * quant) / quant) if quant else (lambda x: x)
    rel = q(rng.uniform(-0.2, 1.2, (B, N, N, R))).astype(np.float32)
    cn = q(rng.uniform(-0.1, 1.1, (B, N, N, 1))).astype(np.float32) if conn else None
    obj = q(rng.uniform(0.3, 1.0, (B, Gp))).astype(np.float32)
    qof = np.full((B, Gp), -1, np.int32)
    for b in range(B):
        M = matched[b]
        qof[b, np.sort(rng.choice(Gp, M, replace=False))] = rng.permutation(N)[:M]
    return (torch.from_numpy(rel), None if cn is None else torch.from_numpy(cn), torch.from_numpy(qof),
            torch.from_numpy(obj))


def definition_cases():
    """name -> (pred_rel, pred_conn, query_of, obj_score, K): the corners of the definition."""
    cases = {}
    cases["ties_across_rank_K"] = random_inputs(1, 2, 8, 6, 7, (6, 7), quant=4) + (20,)
    rel, cn, qof, obj = random_inputs(2, 1, 8, 6, 7, (6,))
    cases["all_scores_zero"] = (torch.full_like(rel, -1.0), cn, qof, obj, 20)
    rel, cn, qof, obj = random_inputs(3, 2, 8, 6, 7, (6, 5), quant=8)
    rel.view(-1)[::7] = float("nan")
    rel.view(-1)[3::11] = -0.0
    cn.view(-1)[5::13] = float("nan")
    g0 = int(torch.nonzero(qof[0] >= 0)[0])
    obj[0, g0] = -0.0                          # every score on that object is -0 or NaN
    cases["nan_and_negative_zero"] = (rel, cn, qof, obj, 150)
    cases["K_1"] = random_inputs(4, 2, 8, 6, 7, (6, 3)) + (1,)
    cases["K_above_domain"] = random_inputs(5, 2, 8, 6, 7, (3, 2), conn=False) + (100,)
    cases["M_0_and_1"] = random_inputs(6, 2, 8, 6, 7, (0, 1)) + (20,)
    rel, cn, qof, obj = random_inputs(7, 1, 6, 5, 9, (6,))       # G = N + 2 = 8 (+ 1 padding): two GT objects unmatched
    qof[0, 8] = -1
    cases["unmatched_gt_objects"] = (rel, cn, qof, obj, 40)
    return cases
