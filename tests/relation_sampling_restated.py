"""Helper (no tests): the relation loss with one sampling POLICY per candidate class (csrc/loss.hip, policy_neg / policy_nm of
egtr_relation_loss_f32) restated in numpy -- the random key (Philox4x32-10 + two rounds of a 32-bit mixer, csrc/rel_sample_key.h) and a float64
expectation of ``mult`` / ``grad`` / ``loss_rel`` built on loss_restated._select / relation_expectation.  Shared by
tests/test_relation_sampling_cpu.py and tests/test_gpu_relation_sampling.py.

A policy is ("largest", count), ("random", count) or ("all", None).  Per image: k = min(n_true count, n_class) when n_true > 0,
else 0, for the first two; k = n_class for "all".  A random class takes the k candidates with the largest key(flat),
flat = (qa N + qb) R + r in QUERY order; the keys of an (image, class) are distinct, so there are no ties."""
import functools
import types

import numpy as np

import loss_restated as LR

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
POLICIES = ("largest", "random", "all")


# ------------------------------------------------------------------------------------------------------------------ the key
def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter 4 x uint32, key 2 x uint32."""
    c0, c1, c2, c3 = (int(c) & MASK32 for c in counter)
    k0, k1 = (int(k) & MASK32 for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def lb32(x):
    """uint32 array -> uint32 array, a bijection: xor-shifts and odd multipliers."""
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def class_keys(seed, stream, b, prob):
    """(ka, kb) of image ``b``, class ``prob`` (0 block, 1 outside); seed / stream: any ints, read modulo 2^64."""
    seed, stream = int(seed) & (2 ** 64 - 1), int(stream) & (2 ** 64 - 1)
    w = philox4x32_10((b, prob, stream & MASK32, stream >> 32), (seed & MASK32, seed >> 32))
    return w[0], w[1]


def sample_key(flat, ka, kb):
    flat = np.asarray(flat, dtype=np.uint32)
    return lb32(lb32(flat ^ np.uint32(ka)) + np.uint32(kb))


def top_by_key(cand, k, ka, kb):
    """Boolean mask (shape of ``cand``) of the ``k`` candidates with the largest key of their flat (C-order) index."""
    idx = np.nonzero(np.asarray(cand).reshape(-1))[0]
    sel = np.zeros(cand.size, dtype=bool)
    if k > 0:
        keys = sample_key(idx, ka, kb)
        sel[idx[np.argsort(keys)[::-1][:k]]] = True
    return sel.reshape(cand.shape)


# ------------------------------------------------------------------------------------------------------------- the selection
def class_count(policy, n_true, n_class):
    name, count = policy
    if name == "all":
        return n_class
    return min(n_true * count, n_class) if n_true > 0 else 0


def select(pred_rel, dense, pred_idx, tgt_idx, negatives, nonmatching, seed=0, stream=0, b=0, order="key"):
    """One image: loss_restated._select's namespace (mult, t, matched, cand, n_true) with ``sel`` / ``k`` by the two policies."""
    for name, _ in (negatives, nonmatching):
        if name not in POLICIES:
            raise ValueError(name)
    s = LR._select(pred_rel, dense, pred_idx, tgt_idx, 0, 0, order)     # k = 0: the true relations, the candidate masks
    mult, sels, ks, free = s.mult.copy(), [], [], np.zeros(s.mult.shape, dtype=bool)
    rank = LR._rank(np.asarray(pred_rel).reshape(-1), order).reshape(pred_rel.shape)
    for prob, (policy, cand) in enumerate(zip((negatives, nonmatching), s.cand)):
        k = class_count(policy, s.n_true, int(cand.sum()))
        if policy[0] == "all":
            sel = cand.copy()
        elif policy[0] == "random":
            sel = top_by_key(cand, k, *class_keys(seed, stream, b, prob))
        else:
            sel = LR.topk_lowest_index_first(pred_rel, cand, k, order)
            if k:   # candidates tied at the threshold, when more of them exist than are taken: the ticket route may take others
                tied = cand & (rank == np.sort(rank[cand])[::-1][k - 1])
                if int(tied.sum()) > int((tied & sel).sum()):
                    free |= tied
        assert int(sel.sum()) == k
        mult += sel
        sels.append(sel)
        ks.append(k)
    return types.SimpleNamespace(mult=mult, t=s.t, matched=s.matched, cand=s.cand, sel=sels, k=ks, n_true=s.n_true, free=free)


def expectation(case, negatives, nonmatching, seed=0, stream=0, order="key"):
    """float64, the whole batch, like loss_restated.relation_expectation: mult [B, N, N, R], grad = mult (sigmoid(x) - y) /
    total, loss_rel, total, unit, images; ``free``: the candidates of a `largest` class tied at its threshold where the tie rule
    decides (the lowest-index rule of the deterministic entry is what ``mult`` holds; the ticket entry may take others of them)."""
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))  # noqa: E731
    N = case["N"]
    mults, ys, images = [], [], []
    for b in range(case["B"]):
        pi, ti = case["indices"][b][0].numpy(), case["indices"][b][1].numpy()
        s = select(case["pred_rel"][b].numpy(), case["dense"][b].numpy(), pi, ti, negatives, nonmatching, seed, stream, b, order)
        w = np.full(N, 1.0 - sig(LR.NM_COST))
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
    return types.SimpleNamespace(mult=mult, grad=mult * unit, loss_rel=loss, total=total, unit=unit, images=images,
                                 free=np.stack([s.free for s in images]))


# ------------------------------------------------------------------------------------------------------------------ inputs
UNIFORM_N, UNIFORM_R, UNIFORM_MATCHED = 6, 3, (1, 3, 4)
UNIFORM_SEEDS = (0, 1234, 2 ** 63 + 5)
UNIFORM_KS = ((8, 8), (1, 40))
UNIFORM_B, UNIFORM_STREAMS = 256, 16


@functools.lru_cache(maxsize=None)
def uniform_case(B=UNIFORM_B):
    """N = 6, R = 3, matched queries {1, 3, 4}, one true relation per image: 26 false candidates in the block, 81 elements outside
    it.  Every image of the batch has the same matching and target (the key depends on the image index); tie-free logits whose
    selected gradients are never 0."""
    rng = np.random.default_rng(4600)
    N, R = UNIFORM_N, UNIFORM_R
    pred = np.array(UNIFORM_MATCHED)
    images = [(pred, np.array([2, 0, 1]), [[0, 1, 2]]) for _ in range(B)]
    return LR.build_case(rng, LR.distinct_logits(rng, B, N, N, R), images)


def uniform_candidates():
    """(flat indices of the 26 block candidates, of the 81 outside elements) of the uniform case, query order."""
    c = uniform_case(1)
    s = LR._select(c["pred_rel"][0].numpy(), c["dense"][0].numpy(), c["indices"][0][0].numpy(), c["indices"][0][1].numpy(), 0, 0,
                   "key")
    assert s.n_true == 1
    return tuple(np.nonzero(m.reshape(-1))[0] for m in s.cand)


@functools.lru_cache(maxsize=None)
def geometry_case(which):
    """"odd": N = 23, R = 13, T = 9 -- rows of 299 elements (a second 256-wide step), R not a power of two.  "rows": N = 260, R = 3
    -- more than 256 rows: the tie-count prefix of the deterministic route, three-valued logits (ties) for the `largest` class;
    ``count_neg``: the block's sample count whose cut falls in a row >= 256."""
    if which == "odd":
        rng = np.random.default_rng(4601)
        N, R, T = 23, 13, 9
        pred = np.sort(rng.choice(N, T, replace=False))
        images = [(pred, rng.permutation(T), [[0, 1, 2], [8, 3, 12], [4, 4, 0]]),
                  (np.array([22, 0, 7]), rng.permutation(3), [[2, 1, 5]])]
        return LR.build_case(rng, LR.distinct_logits(rng, 2, N, N, R), images)
    if which == "rows":
        rng = np.random.default_rng(4602)
        N, R = 260, 3
        pred = np.array([3, 40, 90, 130, 170, 200, 230, 250, 257, 259])
        c = LR.build_case(rng, LR.three_valued(rng, 1, N, N, R), [(pred, rng.permutation(10), [[7, 1, 2], [0, 9, 1]])])
        # the count of the block's `largest` class for which all but one or two of the candidates tied at 0.0 are taken: the
        # last one taken lies in a row >= 256 (n_true = 2, so k = 2 count)
        x = c["pred_rel"][0].numpy()
        sel = LR._select(x, c["dense"][0].numpy(), pred, c["indices"][0][1].numpy(), 0, 0, "key")
        assert sel.n_true == 2
        k = int((sel.cand[0] & (x >= 0.0)).sum()) - 1
        c["count_neg"] = (k - k % 2) // 2
        return c
    raise ValueError(which)


@functools.lru_cache(maxsize=None)
def wide_case():
    """R = 70 (two words per pair), N = 8, B = 2; triplets with predicates on both sides of 64."""
    rng = np.random.default_rng(4603)
    N, R = 8, 70
    images = [(np.array([6, 1, 3, 4]), rng.permutation(4), [[0, 1, 69], [3, 2, 5], [1, 1, 64]]),
              (np.array([0, 7]), rng.permutation(2), [[1, 0, 63]])]
    return LR.build_case(rng, LR.distinct_logits(rng, 2, N, N, R), images)
