"""CPU: the scene-graph evaluator's host path (egtr_amd.evaluation) against the reference's recorded sgdet evaluators
(tests/golden/sgg_eval.npz, make_golden_sgg_eval.py): per-image recalls bit-equal, metrics within 1e-12."""
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import sgg_eval_inputs as SI  # noqa: E402

from egtr_amd.evaluation import SceneGraphRecall, first_ranks_host, gt_entry, numpy_argmax  # noqa: E402

KS = (20, 50, 100)


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "sgg_eval.npz"))


def recorded(g, mode, prefix=""):
    """(candidates, targets) of the fixture: the reference's own pred_entry per image and the seeded targets."""
    _, targets, _ = SI.sgg_eval_inputs(seed=int(g["seed"]), chain=bool(prefix))
    cands = []
    for j in range(len(targets)):
        cands.append({"pred_boxes": torch.from_numpy(g[f"{prefix}{j}_pred_boxes"]),
                      "pred_classes": torch.from_numpy(g[f"{prefix}{j}_pred_classes"]),
                      "pred_rel_inds": torch.from_numpy(g[f"{prefix}{mode}{j}_pred_rel_inds"]),
                      "rel_scores": torch.from_numpy(g[f"{prefix}{mode}{j}_rel_scores"])})
    return cands, targets


def run(cands, targets, mode, bs=16, **kw):
    ev = SceneGraphRecall(SI.R, multiple_preds=(mode == "m"), **kw)
    for i in range(0, len(cands), bs):
        ev.update(cands[i:i + bs], targets[i:i + bs])
    return ev


def test_gt_entry_matches_reference(g):
    _, targets, _ = SI.sgg_eval_inputs(seed=int(g["seed"]))
    for j, t in enumerate(targets):
        e = gt_entry(t)
        assert np.array_equal(e["gt_relations"].numpy(), g[f"{j}_gt_relations"])
        assert np.array_equal(e["gt_boxes"].numpy(), g[f"{j}_gt_boxes"])
        assert np.array_equal(e["gt_classes"].numpy(), g[f"{j}_gt_classes"])


@pytest.mark.parametrize("prefix", ["", "chain_"])
@pytest.mark.parametrize("mode", ["m", "s"])
def test_host_path_matches_reference(g, mode, prefix):
    cands, targets = recorded(g, mode, prefix)
    ev = run(cands, targets, mode, keep_per_image=True)
    assert np.array_equal(ev.per_image().numpy(), g[f"{prefix}{mode}_recall"])      # bit-equal per-image recalls
    want = g[f"{prefix}{mode}_stats"]
    got = ev.compute()
    for j, k in enumerate(KS):
        assert abs(got[f"R@{k}"] - want[j]) <= 1e-12
    mr = ev.mean_recall()
    for j, k in enumerate(KS):
        assert abs(mr[f"mR@{k}"] - g[f"{prefix}{mode}_mr"][j]) <= 1e-12
    per = ev.per_predicate()
    ps = g[f"{prefix}{mode}_pred_stats"]
    for p in range(SI.R):
        for j, k in enumerate(KS):
            if math.isnan(ps[p, j]):
                assert math.isnan(per[p][f"R@{k}"])
            else:
                assert abs(per[p][f"R@{k}"] - ps[p, j]) <= 1e-12
    # the per-image per-predicate recalls the kernel / host path write are the reference's, bit for bit
    nk = len(KS)
    acc_rows = []
    for c, t in zip(cands, targets):
        e = SceneGraphRecall(SI.R, multiple_preds=(mode == "m"))
        e.update([c], [t])
        acc_rows.append(e.acc)
    want_pp = g[f"{prefix}{mode}_pred_recall"]
    for j, a in enumerate(acc_rows):
        for p in range(SI.R):
            if a[e._fbase + p] == 0:
                assert np.isnan(want_pp[p, j]).all()
            else:
                assert np.array_equal(a[e._pbase + p * nk:e._pbase + (p + 1) * nk].numpy(), want_pp[p, j])


def test_metrics_are_nontrivial(g):
    rec = g["s_recall"]
    inside = ((rec[:, 0] > 0) & (rec[:, 0] < rec[:, 1]) & (rec[:, 1] < rec[:, 2]) & (rec[:, 2] < 1)).sum()
    assert inside >= 3
    assert np.isnan(g["m_pred_stats"][-1]).all()       # a predicate that never occurs


def test_mean_recall_nan_quirk():
    ev = SceneGraphRecall(4, ks=(1, 2))
    # one image, one GT triplet of predicate 0 matched at rank 0, one of predicate 1 unmatched
    t = {"class_labels": torch.tensor([0, 1, 2]), "boxes": torch.tensor([[0.25, 0.25, 0.1, 0.1]] * 3),
         "rel": torch.zeros(3, 3, 4), "orig_size": torch.tensor([100, 100])}
    t["rel"][0, 1, 0] = 1
    t["rel"][0, 2, 1] = 1
    boxes = torch.tensor([[20.0, 20.0, 30.0, 30.0]] * 3)
    c = {"pred_boxes": boxes, "pred_classes": torch.tensor([0, 1, 2]), "pred_rel_inds": torch.tensor([[0, 1]]),
         "rel_scores": torch.tensor([[0.9, 0.1, 0.0, 0.0]])}
    ev.update([c], [t])
    per = ev.per_predicate()
    assert per[0] == {"R@1": 1.0, "R@2": 1.0} and per[1] == {"R@1": 0.0, "R@2": 0.0}
    assert math.isnan(per[2]["R@1"]) and math.isnan(per[3]["R@2"])
    assert ev.mean_recall() == {"mR@1": 0.25, "mR@2": 0.25}      # (1 + 0) / 4 predicates, NaNs left out of the sum
    assert ev.compute() == {"R@1": 0.5, "R@2": 0.5}


def test_numpy_argmax_semantics():
    rows = torch.tensor([[0.1, 0.5, 0.5, 0.2], [0.1, float("nan"), 0.9, float("nan")], [float("-inf")] * 4,
                         [0.3, 0.3, 0.3, 0.3]])
    assert numpy_argmax(rows).tolist() == np.argmax(rows.numpy(), 1).tolist() == [1, 1, 0, 0]


@pytest.mark.parametrize("mode", ["m", "s"])
def test_merge_equals_one_pass(g, mode):
    cands, targets = recorded(g, mode)
    whole = run(cands, targets, mode)
    a = run(cands[:7], targets[:7], mode)
    b = run(cands[7:], targets[7:], mode)
    a.merge(b)
    assert torch.allclose(a.acc, whole.acc, rtol=0, atol=1e-12)
    for k, v in whole.compute().items():
        assert abs(a.compute()[k] - v) <= 1e-12


@pytest.mark.parametrize("mode", ["m", "s"])
def test_batch_size_independent(g, mode):
    cands, targets = recorded(g, mode)
    accs = [run(cands, targets, mode, bs=bs).acc for bs in (1, 3, 16)]
    assert torch.equal(accs[0], accs[1]) and torch.equal(accs[0], accs[2])


def test_zero_gt_image_is_skipped(g):
    cands, targets = recorded(g, "s")
    empty = dict(targets[0], rel=torch.zeros_like(targets[0]["rel"]))
    ev = run(cands[:3], targets[:3], "s", keep_per_image=True)
    ev2 = SceneGraphRecall(SI.R, keep_per_image=True)
    ev2.update(cands[:1] + [cands[0]] + cands[1:3], targets[:1] + [empty] + targets[1:3])
    assert ev2.skipped == 1 and ev2.n_images == 3 and ev.skipped == 0
    assert torch.equal(ev2.acc[:3], ev.acc[:3]) and torch.equal(ev2.per_image(), ev.per_image())


def test_first_ranks_host_small():
    gt_rels = torch.tensor([[0, 1, 2], [1, 0, 2]])
    gt_boxes = torch.tensor([[0.0, 0.0, 9.0, 9.0], [20.0, 0.0, 29.0, 9.0]])
    gt_cls = torch.tensor([3, 4])
    # candidate 0: wrong predicate; 1: matches GT 0; 2: matches GT 0 again; GT 1 never
    pred = torch.tensor([[0, 1, 1], [0, 1, 2], [0, 1, 2]])
    fr = first_ranks_host(pred, gt_boxes, gt_cls, gt_rels, gt_boxes, gt_cls)
    assert fr.tolist() == [1, 3]


def test_bad_arguments(g):
    with pytest.raises(ValueError):
        SceneGraphRecall(0)
    with pytest.raises(ValueError):
        SceneGraphRecall(300)
    with pytest.raises(ValueError):
        SceneGraphRecall(5, ks=(50, 20))
    with pytest.raises(ValueError):
        SceneGraphRecall(5, ks=tuple(range(1, 11)))
    with pytest.raises(ValueError):
        SceneGraphRecall(5, iou_thresh=float("nan"))
    cands, targets = recorded(g, "s")
    ev = SceneGraphRecall(SI.R)
    with pytest.raises(ValueError):
        ev.update(cands[:2], targets[:1])
    with pytest.raises(KeyError):
        ev.update([{k: v for k, v in cands[0].items() if k != "rel_scores"}], targets[:1])
    with pytest.raises(ValueError):
        ev.update([dict(cands[0], rel_scores=cands[0]["rel_scores"][:, :3])], targets[:1])
    with pytest.raises(ValueError):
        SceneGraphRecall(3).update(cands[:1], targets[:1])      # GT predicates beyond num_rel_labels
    with pytest.raises(RuntimeError):
        ev.per_image()
    with pytest.raises(ValueError):
        ev.merge(SceneGraphRecall(SI.R, multiple_preds=True))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, world, port, path, q):
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(HERE, "golden"))
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        g = np.load(path)
        cands, targets = recorded(g, "m")
        half = len(cands) // 2
        sl = slice(0, half) if rank == 0 else slice(half, None)
        ev = run(cands[sl], targets[sl], "m")
        ev.all_reduce()
        q.put((rank, ev.acc.numpy()))
    finally:
        dist.destroy_process_group()


def test_all_reduce_two_ranks_gloo(g):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, os.path.join(HERE, "golden", "sgg_eval.npz"), q))
             for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    cands, targets = recorded(g, "m")
    a = run(cands[:8], targets[:8], "m")
    a.merge(run(cands[8:], targets[8:], "m"))
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], a.acc.numpy())
