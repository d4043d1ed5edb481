"""GPU: the phrase- and predicate-detection kernels (csrc/vrd_eval.hip) and the device paths of
egtr_amd.evaluation.vrd -- per-image recalls bit-equal to the reference's recorded VRD evaluators
(tests/golden/vrd_eval.npz), first ranks index-exact and accumulators bit-equal to the host path, the hand-made images
of vrd_eval_inputs.py, merge / batch-size independence, the zero-shot pass on the phrdet first ranks,
runtime.matched_pair_candidates, and the kernel's own answer to more GT relations than it keeps in LDS."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import vrd_eval_inputs as VI  # noqa: E402

from egtr_amd import _lib  # noqa: E402
from egtr_amd.deformable_detr import DeformableDetrHungarianMatcher  # noqa: E402
from egtr_amd.evaluation import (PhraseDetectionRecall, PredicateDetectionRecall, SceneGraphRecall, gt_entry,  # noqa: E402
                                 phrase_first_ranks_host)
from egtr_amd.kernels.vrd import NO_RANK, PREDDET_MAX_GT  # noqa: E402
from egtr_amd.runtime import matched_pair_candidates  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KS = (1, 20, 50, 100)         # k = 100 > K = 65 occurs
CLASSES = {"phrdet": PhraseDetectionRecall, "preddet": PredicateDetectionRecall}
GROUPS = ((0, 8), (8, 12))    # K = 100, K = 65


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "vrd_eval.npz"))


@pytest.fixture(scope="module")
def inputs(g):
    targets, phr, prd = VI.vrd_eval_inputs(int(g["seed"]))
    to = lambda entries: [{k: torch.from_numpy(v) for k, v in e.items()} for e in entries]  # noqa: E731
    return targets, {"phrdet": to(phr), "preddet": to(prd)}


def on(cands, device=DEV):
    return [{k: v.to(device) for k, v in c.items()} for c in cands]


def run(mode, cands, targets, groups=GROUPS, device=DEV, ks=KS, R=VI.R, **kw):
    """The evaluator after one update per group, with ``ranks``: the per-triplet outputs of every update, concatenated --
    [first_rank] for phrdet, [first_rank, chosen_row, first_rank_pred] for preddet."""
    ev = CLASSES[mode](R, ks=ks, **kw)
    ranks = []
    for lo, hi in groups:
        ev.update(on(cands[lo:hi], device), targets[lo:hi])
        if mode == "preddet":
            ranks.append([ev.last_first_rank, ev.last_chosen_row, ev.last_first_rank_pred])
        elif device.type == "cpu":       # the host path of phrdet keeps no ranks: ask the host matching itself
            es = [gt_entry(t) for t in targets[lo:hi]]
            ranks.append([torch.cat([phrase_first_ranks_host(
                c["pred_rel_inds"], c["pred_boxes"], c["pred_classes"], e["gt_relations"], e["gt_boxes"],
                e["gt_classes"]) for c, e in zip(cands[lo:hi], es)])])
        else:
            ranks.append([ev.last_first_rank])
    ev.ranks = [torch.cat([r.cpu().long() for r in rs]) for rs in zip(*ranks)]
    return ev


@pytest.mark.parametrize("mode", ["phrdet", "preddet"])
def test_device_matches_reference_and_host(g, inputs, mode):
    targets, cands = inputs
    ev = run(mode, cands[mode], targets, keep_per_image=True)
    host = run(mode, cands[mode], targets, device=torch.device("cpu"), keep_per_image=True)
    assert np.array_equal(ev.per_image().numpy(), g[f"{mode}_recall"])           # the reference's, bit for bit
    for got, want in zip(ev.ranks, host.ranks):                                 # index-exact
        assert torch.equal(got, want)
    assert 64 in ev.ranks[1 if mode == "preddet" else 0].tolist()               # lane 0 of the second 64-candidate step
    assert torch.equal(ev.acc.cpu(), host.acc)                                  # same rows, same fold: bit-equal
    got = ev.compute()
    for j, k in enumerate(KS):
        assert abs(got[f"R@{k}"] - g[f"{mode}_stats"][j]) <= 1e-12
    for j, k in enumerate(KS[1:]):
        assert abs(got[f"mR@{k}"] - g[f"{mode}_mr"][j]) <= 1e-12
    if mode == "preddet":    # the image without candidates counts with recall 0 (its pairs were padded to the batch's K)
        assert ev.n_images == 12 and (ev.per_image()[VI.NO_CAND] == 0).all()


@pytest.mark.parametrize("mode", ["phrdet", "preddet"])
def test_batch_of_three_with_an_image_without_gt(inputs, mode):
    targets, cands = inputs
    empty = dict(targets[8], rel=torch.zeros_like(targets[8]["rel"]))
    cs, ts = [cands[mode][8], cands[mode][8], cands[mode][9]], [targets[8], empty, targets[9]]
    ev = run(mode, cs, ts, groups=((0, 3),), keep_per_image=True)
    host = run(mode, cs, ts, groups=((0, 3),), device=torch.device("cpu"), keep_per_image=True)
    assert ev.skipped == 1 and ev.n_images == 2
    assert torch.equal(ev.acc.cpu(), host.acc) and torch.equal(ev.per_image(), host.per_image())
    one = run(mode, cs, ts, groups=((0, 1), (1, 2), (2, 3)))                    # batch size 1 x 3 = batch size 3
    assert torch.equal(one.acc, ev.acc)


def _four_relations(target):
    """The target with 4 of its GT relations, at most 2 of one predicate: every recall of the image is then a multiple of
    1/4 (or 1/2, 1/1 per predicate), and sums of such values are exact in float64 whatever their order."""
    keep, count = [], {}
    for s, o, p in target["rel"].nonzero().tolist():
        if count.get(p, 0) < 2 and len(keep) < 4:
            keep.append((s, o, p))
            count[p] = count.get(p, 0) + 1
    assert len(keep) == 4
    rel = torch.zeros_like(target["rel"])
    for s, o, p in keep:
        rel[s, o, p] = 1
    return dict(target, rel=rel)


@pytest.mark.parametrize("mode", ["phrdet", "preddet"])
def test_merge_of_two_halves_equals_one_pass(inputs, mode):
    """``merge`` adds the accumulators, so "two halves merged" is (r0 + r1) + (r2 + r3) where one pass is
    ((r0 + r1) + r2) + r3.  That is the same float64 bit for bit exactly when the additions do not round, so the images
    here have recalls that are multiples of 1/4; on the whole fixture, whose recalls are ninths and sevenths, the two
    differ in the last bit (tests/test_vrd_eval_cpu.py::test_merge_and_batch_size bounds that with the sgdet tolerance)."""
    targets, cands = inputs
    pick = (0, 2, 4, 6)
    cs, ts = [cands[mode][i] for i in pick], [_four_relations(targets[i]) for i in pick]
    whole = run(mode, cs, ts, groups=((0, 4),))
    a = run(mode, cs, ts, groups=((0, 2),))
    a.merge(run(mode, cs, ts, groups=((2, 4),)))
    assert torch.equal(a.acc, whole.acc)
    assert 0 < whole.compute()["R@100"] <= 1 and whole.n_images == 4
    host = run(mode, cs, ts, groups=((0, 4),), device=torch.device("cpu"))
    assert torch.equal(whole.acc.cpu(), host.acc)


def test_phrdet_hand_image_on_device():
    cand, target, want, K = VI.phrdet_hand_image()
    ev = run("phrdet", [cand], [target], groups=((0, 1),), ks=(1, 2, 3), R=4)
    assert ev.ranks[0].tolist() == want       # union IoU 0.85 hits, exactly 0.5 hits (>=), 0.49 misses
    sg = SceneGraphRecall(4, ks=(1, 2, 3), multiple_preds=True)
    sg.update(on([cand]), [target])
    assert sg.last_first_rank.tolist()[0] == K      # the sgdet kernel misses triplet 0: its subject IoU is 0.25
    assert ev.compute()["R@3"] == 2 / 3


def test_preddet_hand_image_on_device():
    cand, target, rows, fr, fr_pred = VI.preddet_hand_image()
    none = lambda xs: [NO_RANK if x is None else x for x in xs]  # noqa: E731
    ev = run("preddet", [cand], [target], groups=((0, 1),), ks=(1, 4, 7, 9), R=4)
    assert ev.ranks[1].tolist() == rows       # fall-back to row 0, a GT pair with two predicates
    assert ev.ranks[0].tolist() == none(fr)   # the tie rule: equal scores in ascending flat index
    assert ev.ranks[2].tolist() == none(fr_pred)      # ranks inside the rows of one predicate differ from the global ones
    host = run("preddet", [cand], [target], groups=((0, 1),), device=torch.device("cpu"), ks=(1, 4, 7, 9), R=4)
    assert torch.equal(ev.acc.cpu(), host.acc)
    assert ev.compute() == host.compute()


def _stress(seed, B, K, R, G, T):
    """Random preddet images with quantised scores (many ties), NaN / signed-zero scores, repeated and absent GT pairs."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cands, targets = [], []
    for b in range(B):
        rel = torch.zeros(G, G, R)
        for _ in range(T):
            s, o = rng.choice(G, 2, replace=False)
            rel[int(s), int(o), int(rng.integers(0, R))] = 1
        boxes = torch.tensor([[0.25, 0.25, 0.125, 0.125]] * G)
        targets.append(dict(class_labels=torch.arange(G), boxes=boxes, rel=rel, orig_size=torch.tensor([64, 64])))
        sc = (np.round(rng.random((K, R)) * 8) / 8).astype(np.float32)
        sc[rng.random((K, R)) < 0.02] = np.nan
        sc[rng.random((K, R)) < 0.02] = -0.0
        pairs = rng.integers(0, G, (K, 2))
        pairs[rng.random(K) < 0.05] = -1                      # out of range: never chosen by a valid GT pair
        cands.append(dict(pred_rel_inds=torch.from_numpy(pairs), rel_scores=torch.from_numpy(sc)))
    return cands, targets


@pytest.mark.parametrize("K,R,G,T", [(100, 51, 8, 30), (65, 256, 9, 60)])
def test_preddet_ties_and_streaming_path_equal_host(K, R, G, T):
    # second case: n_gt * R > 8192, so the order keys do not fit in LDS and are read from rel_scores
    cands, targets = _stress(7 + K, 3, K, R, G, T)
    ev = run("preddet", cands, targets, groups=((0, 3),), ks=(1, 5, 50, 500), R=R)
    host = run("preddet", cands, targets, groups=((0, 3),), device=torch.device("cpu"), ks=(1, 5, 50, 500), R=R)
    if R == 256:
        assert max(int(t["rel"].sum()) for t in targets) * R > 8192
    for got, want in zip(ev.ranks, host.ranks):
        assert torch.equal(got, want)
    assert (host.ranks[0] < NO_RANK).sum() > 10 and (host.ranks[0] != host.ranks[2]).any()
    assert torch.equal(ev.acc.cpu(), host.acc)


def test_preddet_kernel_with_too_many_gt_relations():
    """evaluation/vrd.py rejects an image with more than PREDDET_MAX_GT relations, so only a direct call reaches the
    kernel's own answer: NaN recalls, correct counted / skipped / presence columns, NO_RANK and row 0 per triplet --
    and the neighbouring image's row untouched."""
    K, R, ks, n0 = 4, 3, (1, 2), PREDDET_MAX_GT + 1
    nk = len(ks)
    gen = torch.Generator().manual_seed(11)
    pairs = torch.tensor([[[0, 1], [1, 2], [2, 0], [0, 1]], [[0, 1], [1, 2], [0, 1], [2, 0]]])
    scores = torch.rand(2, K, R, generator=gen)
    cyc = torch.tensor([[0, 1, 0], [1, 2, 2], [2, 0, 0]])        # three objects, predicates 0 and 2; predicate 1 is absent
    rels0 = cyc[torch.arange(n0) % 3]
    rels1 = torch.tensor([[0, 1, 1], [1, 2, 0]])

    def launch(rels, sizes, lo, hi):
        # the C entry itself, as ops.sgg_eval_preddet calls it, but into PREFILLED outputs: a row the kernel does not
        # write keeps the 7 (ops allocates with torch.empty, where an unwritten chosen_row could happen to read 0)
        off = torch.tensor([0] + sizes).cumsum(0).to(DEV)
        box_off = (3 * torch.arange(len(sizes) + 1)).to(DEV)
        T, d_rels = int(off[-1]), rels.to(DEV)
        d_pairs, d_scores = pairs[lo:hi].to(DEV), scores[lo:hi].to(DEV)
        slab = torch.full((hi - lo, nk + 2 + R * (nk + 1)), 7.0, dtype=torch.float64, device=DEV)
        out = torch.full((3, T), 7, dtype=torch.int32, device=DEV)
        _lib.launch("egtr_sgg_eval_preddet_f32", d_pairs.data_ptr(), d_scores.data_ptr(), hi - lo, K, R,
                    d_rels.data_ptr(), off.data_ptr(), T, box_off.data_ptr(), 3 * len(sizes), (ctypes.c_int * nk)(*ks),
                    nk, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), slab.data_ptr(), None)
        return [slab.cpu()] + [x.cpu() for x in out]      # slab, chosen_row, first_rank, first_rank_pred

    slab, rows, fr, fr_pred = launch(torch.cat([rels0, rels1]), [n0, 2], 0, 2)
    alone = launch(rels1, [2], 1, 2)
    bad, pbase, fbase = slab[0], nk + 2, nk + 2 + R * nk
    assert bad[:nk].isnan().all()
    assert bad[nk] == 1 and bad[nk + 1] == 0                    # counted, not skipped
    for p, present in enumerate((True, False, True)):
        cols = bad[pbase + p * nk:pbase + (p + 1) * nk]
        assert cols.isnan().all() if present else (cols == 0).all()
        assert bad[fbase + p] == (1.0 if present else 0.0)
    assert (fr[:n0] == NO_RANK).all() and (fr_pred[:n0] == NO_RANK).all() and (rows[:n0] == 0).all()
    assert torch.equal(slab[1], alone[0][0]) and not slab[1].isnan().any() and slab[1][nk] == 1
    for got, want in zip((rows, fr, fr_pred), alone[1:]):
        assert torch.equal(got[n0:], want)


def test_phrdet_zero_shot_equals_host(inputs):
    targets, cands = inputs
    rng = np.random.Generator(np.random.PCG64(3))
    fg = torch.from_numpy((rng.random((21, 21, VI.R)) < 0.5).astype(np.int64))   # half of the triplets "seen"
    ev = run("phrdet", cands["phrdet"], targets, train_counts=fg)
    host = run("phrdet", cands["phrdet"], targets, device=torch.device("cpu"), train_counts=fg)
    assert host.n_zero_shot_triplets > 10 and torch.equal(ev.zs_acc.cpu(), host.zs_acc)
    assert ev.zero_shot() == host.zero_shot() and set(ev.compute()) >= {f"zR@{k}" for k in KS}
    assert 0 < host.zero_shot()["zR@100"] < 1


def test_matched_pair_candidates_tiny():
    torch.manual_seed(5)
    B, N, G, R, C = 2, 6, 3, 4, 5
    outputs = {"logits": torch.randn(B, N, C + 1, device=DEV), "pred_boxes": torch.rand(B, N, 4, device=DEV) * 0.4 + 0.3,
               "pred_rel": torch.rand(B, N, N, R, device=DEV) * 1.4 - 0.2,
               "pred_connectivity": torch.rand(B, N, N, 1, device=DEV) * 1.4 - 0.2}
    targets = [dict(class_labels=torch.randint(0, C, (G,)), boxes=torch.rand(G, 4) * 0.4 + 0.3) for _ in range(B)]
    matcher = DeformableDetrHungarianMatcher(class_cost=2.0, bbox_cost=5.0, giou_cost=2.0)
    got = matched_pair_candidates(outputs, targets, matcher, C)
    matched = matcher({"logits": outputs["logits"][..., :C], "pred_boxes": outputs["pred_boxes"]}, targets)[0]
    for b in range(B):                        # the plain restatement: loops over ordered GT pairs
        q_of = {int(t): int(q) for q, t in zip(matched[b][0].tolist(), matched[b][1].tolist())}
        assert sorted(q_of) == list(range(G))
        pairs = [(s, o) for s in range(G) for o in range(G) if s != o]
        rel = outputs["pred_rel"][b].clamp(0, 1) * outputs["pred_connectivity"][b].clamp(0, 1)
        want = torch.stack([rel[q_of[s], q_of[o]] for s, o in pairs])
        assert got[b]["pred_rel_inds"].tolist() == [list(p) for p in pairs]
        assert torch.equal(got[b]["rel_scores"], want)
    tg = [dict(t, rel=torch.zeros(G, G, R), orig_size=torch.tensor([64, 64])) for t in targets]
    tg[0]["rel"][0, 1, 2] = tg[0]["rel"][2, 0, 1] = tg[1]["rel"][1, 2, 3] = 1
    ev, host = PredicateDetectionRecall(R, ks=(1, 4)), PredicateDetectionRecall(R, ks=(1, 4))
    ev.update(got, tg)
    host.update([{k: v.cpu() for k, v in c.items()} for c in got], tg)
    assert torch.equal(ev.acc.cpu(), host.acc) and ev.n_images == 2
