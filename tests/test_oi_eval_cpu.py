"""CPU: the Open Images relation metrics' host path (egtr_amd.evaluation.OpenImagesRelationMetrics) against the
reference's recorded OI evaluator (tests/golden/oi_eval.npz, make_golden_oi_eval.py): selected detections, per-image
recalls and TP flags bit-equal, metrics within 1e-12; tie rules, skipped images, batching, merge and all_gather."""
import ctypes
import hashlib
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import oi_eval_inputs as OI  # noqa: E402

from egtr_amd import _lib  # noqa: E402
from egtr_amd.evaluation import OpenImagesRelationMetrics, oi_select_host  # noqa: E402

KS = (1, 5, 10, 20, 50, 100)
R = OI.R


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "oi_eval.npz"))


def recorded(g, device="cpu"):
    """(candidates, targets) of the fixture: the reference's pred_entry per image (pred_scores rebuilt from the seeded
    model outputs exactly as evaluate_batch does, and pinned by the recorded digest) and the seeded targets."""
    outputs, targets, _ = OI.oi_eval_inputs(seed=int(g["seed"]))
    rel = torch.clamp(outputs["pred_rel"], 0.0, 1.0) * torch.clamp(outputs["pred_connectivity"], 0.0, 1.0)
    B, N = rel.shape[:2]
    pairs = torch.cartesian_prod(torch.arange(N), torch.arange(N))
    cands = []
    for j in range(B):
        ps = rel[j].reshape(N * N, R).contiguous()
        assert hashlib.sha256(ps.numpy().tobytes()).hexdigest() == str(g[f"img{j}_pred_scores_sha256"])
        c = {"pred_boxes": torch.from_numpy(g[f"img{j}_pred_boxes"]),
             "pred_classes": torch.from_numpy(g[f"img{j}_pred_class"]),
             "obj_scores": torch.from_numpy(g[f"img{j}_pred_cls_scores"]), "sbj_obj_inds": pairs, "pred_scores": ps}
        cands.append({k: v.to(device) for k, v in c.items()})
    return cands, targets


def run(cands, targets, batch=4):
    ev = OpenImagesRelationMetrics(R)
    for i in range(0, len(cands), batch):
        ev.update(cands[i:i + batch], targets[i:i + batch])
    return ev


def sorted_records(ev):
    """Records sorted by class, then confidence descending (ties: image order, in-image rank), on the host."""
    p, s, tp = (x.cpu() for x in ev._records())
    key = (p << 32) | (0xFFFFFFFF - (s.view(torch.int32).long() & 0xFFFFFFFF))
    perm = torch.sort(key, stable=True).indices
    return p[perm], s[perm], tp[:, perm]


def check_detections(g, j, sop, score, classes, boxes):
    lab = g[f"det{j}_labels"]
    assert sop.shape[0] == lab.shape[0]
    s, o, p = sop[:, 0].long(), sop[:, 1].long(), sop[:, 2].long()
    assert np.array_equal(classes[s].numpy(), lab[:, 0]) and np.array_equal(p.numpy(), lab[:, 1])
    assert np.array_equal(classes[o].numpy(), lab[:, 2])
    assert np.array_equal(torch.cat([boxes[s], boxes[o]], 1).numpy(), g[f"det{j}_boxes"])
    assert np.array_equal(score.numpy().view(np.uint32), g[f"det{j}_scores"].view(np.uint32))


def check_against_reference(g, ev, rows):
    nk = len(KS)
    # per-image recalls: bit-equal
    assert np.array_equal(rows[:, :nk].numpy(), g["per_image_recall"])
    assert np.array_equal(rows[:, 2 * nk + 3:].sum(0).numpy(), g["npos"].astype(np.float64))
    # TP flags in the reference's sorted order (recovered from its rec), per class and mode; rec / prec bit-equal
    p, s, tp = sorted_records(ev)
    npos = g["npos"]
    for c in range(R):
        sel = p == c
        conf = g[f"cls{c}_confidence"]
        assert np.array_equal(s[sel].double().numpy(), -np.sort(-conf))
        for m, mode in enumerate(("rel", "phr")):
            rec = g[f"cls{c}_{mode}_rec"]
            flags = tp[m, sel].long()
            cum = torch.cumsum(flags, 0).double()
            mine = (cum / (float(npos[c]) + 1e-12)).numpy()
            assert np.array_equal(mine, rec), (c, mode)
            prec = (cum / torch.arange(1, len(cum) + 1, dtype=torch.float64)).numpy()
            assert np.array_equal(prec, g[f"cls{c}_{mode}_prec"]), (c, mode)
    got = ev.compute()
    for k in ("w_rel_mAP", "w_phr_mAP", "rel_mAP", "phr_mAP", "microR@50", "score"):
        assert abs(got[k] - float(g[f"metric_{k}"])) <= 1e-12, k
    for q, k in enumerate(KS):
        assert abs(got[f"R@{k}"] - float(g["per_image_recall"][:, q].mean())) <= 1e-12
    pc = ev.per_class()
    for c in range(R):
        assert abs(pc[c]["rel_AP"] - float(g[f"cls{c}_rel_ap"])) <= 1e-12
        assert abs(pc[c]["phr_AP"] - float(g[f"cls{c}_phr_ap"])) <= 1e-12
        assert pc[c]["npos"] == int(npos[c])
    assert ev.n_images == len(g["per_image_recall"]) and ev.skipped == 0


def test_host_selection_matches_reference(g):
    cands, _ = recorded(g)
    for j, c in enumerate(cands):
        sop, score = oi_select_host(c["pred_scores"], c["obj_scores"], c["sbj_obj_inds"])
        check_detections(g, j, sop, score, c["pred_classes"], c["pred_boxes"])


def test_host_path_matches_reference(g):
    cands, targets = recorded(g)
    ev = OpenImagesRelationMetrics(R)
    rows = []
    for i in range(0, len(cands), 4):
        ev.update(cands[i:i + 4], targets[i:i + 4])
        rows.append(ev.last_rows)
    check_against_reference(g, ev, torch.cat(rows))


def test_fixture_covers_the_edge_cases(g):
    # a class with detections and no GT, a class with GT and no detections, an image cut by the 1e-5 filter, TP and FP
    npos = g["npos"]
    assert any(npos[c] == 0 and len(g[f"cls{c}_confidence"]) for c in range(R))
    assert any(npos[c] > 0 and len(g[f"cls{c}_confidence"]) == 0 for c in range(R))
    assert min(len(g[f"det{j}_scores"]) for j in range(OI.B)) < 100
    assert 0.0 < float(g["metric_w_rel_mAP"]) < 1.0 and 0.0 < float(g["metric_microR@50"]) < 1.0
    # self pairs among the selected detections (equal subject and object boxes)
    assert any((g[f"det{j}_boxes"][:, :4] == g[f"det{j}_boxes"][:, 4:]).all(1).any() for j in range(OI.B))


@pytest.mark.parametrize("batch", [1, 3, 4])
def test_batch_size_independent(g, batch):
    cands, targets = recorded(g)
    a, b = run(cands, targets, batch), run(cands, targets, 20)
    assert torch.equal(a.acc, b.acc)
    assert a.compute() == b.compute()
    for x, y in zip(a._records(), b._records()):
        assert torch.equal(x, y)


def test_merge_equals_one_pass(g):
    cands, targets = recorded(g)
    one = run(cands, targets)
    a = run(cands[:8], targets[:8])
    a.merge(run(cands[8:], targets[8:]))
    for x, y in zip(a._records(), one._records()):
        assert torch.equal(x, y)
    got, ref = a.compute(), one.compute()
    for k, v in ref.items():
        assert got[k] == pytest.approx(v, rel=1e-14, abs=1e-15), k


def _target(boxes, classes, rels, R_=4):
    """A target dict from integer pixel boxes on a 1024 x 512 image and (s, o, p) triplets."""
    cx = [[(b[0] + b[2]) / 2 / 1024, (b[1] + b[3]) / 2 / 512, (b[2] - b[0]) / 1024, (b[3] - b[1]) / 512] for b in boxes]
    rel = torch.zeros(len(boxes), len(boxes), R_)
    for s, o, p in rels:
        rel[s, o, p] = 1.0
    return {"class_labels": torch.tensor(classes), "boxes": torch.tensor(cx, dtype=torch.float32), "rel": rel,
            "orig_size": torch.tensor([512, 1024])}


def _cand(boxes, classes, obj, scores, pairs):
    return {"pred_boxes": torch.tensor(boxes, dtype=torch.float32), "pred_classes": torch.tensor(classes),
            "obj_scores": torch.tensor(obj, dtype=torch.float32),
            "pred_scores": torch.tensor(scores, dtype=torch.float32), "sbj_obj_inds": torch.tensor(pairs)}


def test_tie_rules():
    # equal predicate scores: the lower predicate index ranks first; equal spo: the lower flat index (pair-major)
    scores = torch.tensor([[0.5, 0.7, 0.7, 0.1], [0.7, 0.2, 0.7, 0.7]])
    sop, sc = oi_select_host(scores, torch.ones(2), torch.tensor([[0, 1], [1, 0]]), topk=3, prd_k=2)
    assert sop.tolist() == [[0, 1, 1], [0, 1, 2], [1, 0, 0]]
    assert sc.tolist() == pytest.approx([0.7, 0.7, 0.7])
    # NaN ranks last among a pair's predicates; spo <= 1e-5 is dropped; self pairs are candidates
    scores = torch.tensor([[float("nan"), 0.3, 0.2], [1e-6, 0.0, 0.0]])
    sop, sc = oi_select_host(scores, torch.ones(2), torch.tensor([[0, 0], [1, 1]]), topk=10, prd_k=2)
    assert sop.tolist() == [[0, 0, 1], [0, 0, 2]]


def test_equal_confidences_order_by_image_then_rank():
    # two images, one detection each of class 0 with the same score: the first image's detection is sorted first, so
    # the TP of image 0 and the FP of image 1 give AP 0.5 with npos 2 (the reverse order would give 0.25)
    box = [100, 100, 199, 149]
    far = [600, 300, 699, 349]
    t0 = _target([box, far], [0, 1], [(0, 1, 0)])
    t1 = _target([box, far], [0, 1], [(0, 1, 0)])
    hit = _cand([box, far], [0, 1], [1.0, 1.0], [[0, 0, 0, 0], [0.9, 0, 0, 0]], [[1, 0], [0, 1]])
    miss = _cand([box, far], [0, 0], [1.0, 1.0], [[0, 0, 0, 0], [0.9, 0, 0, 0]], [[1, 0], [0, 1]])
    ev = OpenImagesRelationMetrics(4, prd_k=1)
    ev.update([hit, miss], [t0, t1])
    pc = ev.per_class()
    assert pc[0]["npos"] == 2 and pc[0]["rel_AP"] == pytest.approx(0.5, abs=1e-11)


def test_zero_gt_image_is_skipped_and_zero_ap_classes():
    box = [100, 100, 199, 149]
    far = [600, 300, 699, 349]
    t = _target([box, far], [0, 1], [(0, 1, 0), (1, 0, 2)])
    empty = _target([box, far], [0, 1], [])
    # class 0: detected and matched; class 1: detections, no GT; class 2: GT, no detections
    c = _cand([box, far], [0, 1], [1.0, 1.0], [[0, 0.5, 0, 0], [0.9, 0.4, 0, 0]], [[1, 0], [0, 1]])
    ev = OpenImagesRelationMetrics(4)
    ev.update([c, c], [t, empty])
    assert ev.n_images == 1 and ev.skipped == 1
    pc = ev.per_class()
    assert pc[0]["rel_AP"] == pytest.approx(1.0, abs=1e-11) and pc[0]["npos"] == 1
    assert pc[1]["rel_AP"] == 0.0 and pc[1]["npos"] == 0
    assert pc[2]["rel_AP"] == 0.0 and pc[2]["phr_AP"] == 0.0 and pc[2]["npos"] == 1
    got = ev.compute()
    assert got["microR@100"] == pytest.approx(0.5) and got["R@1"] == pytest.approx(0.5)
    assert got["w_rel_mAP"] == pytest.approx(0.5) and got["rel_mAP"] == pytest.approx(0.25)
    # no image at all: NaN means, zero mAPs
    e = OpenImagesRelationMetrics(4).compute()
    assert math.isnan(e["R@50"]) and e["rel_mAP"] == 0.0


def test_bad_arguments(g):
    for kw in (dict(num_rel_labels=0), dict(num_rel_labels=300), dict(num_rel_labels=5, ks=(50, 20)),
               dict(num_rel_labels=5, topk=0), dict(num_rel_labels=5, topk=2048), dict(num_rel_labels=5, prd_k=9)):
        with pytest.raises(ValueError):
            OpenImagesRelationMetrics(**kw)
    cands, targets = recorded(g)
    ev = OpenImagesRelationMetrics(R)
    with pytest.raises(ValueError):
        ev.update(cands[:2], targets[:1])
    with pytest.raises(KeyError):
        ev.update([{k: v for k, v in cands[0].items() if k != "obj_scores"}], targets[:1])
    with pytest.raises(ValueError):
        ev.update([dict(cands[0], pred_scores=cands[0]["pred_scores"][:, :3])], targets[:1])
    with pytest.raises(ValueError):
        ev.update([dict(cands[0], sbj_obj_inds=cands[0]["sbj_obj_inds"][:5])], targets[:1])
    with pytest.raises(ValueError):
        OpenImagesRelationMetrics(5).update([dict(cands[0], pred_scores=cands[0]["pred_scores"][:, :5])],
                                            targets[:1])   # GT predicates beyond num_rel_labels
    with pytest.raises(ValueError):
        ev.merge(OpenImagesRelationMetrics(R, topk=50))


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    h = _lib.lib()
    ks = (ctypes.c_int * 2)(1, 5)
    assert h.egtr_oi_eval_width(30, 6) == 2 * 6 + 3 + 30
    assert h.egtr_oi_eval_width(0, 6) == -1 and h.egtr_oi_eval_width(30, 9) == -1
    assert h.egtr_oi_select_workspace_bytes(40000, 100, 2, 2) == 2 * 79 * 100 * 8
    assert h.egtr_oi_select_workspace_bytes(90001, 100, 2, 1) == -1
    # (stream, scores, img_stride, row_stride, obj, pairs, pair_stride, B, M, N, R, topk, prd_k, ws, sop, score, count)
    good = [None, 8, 0, 30, 8, None, 0, 1, 4, 2, 30, 100, 2, 8, 8, 8, 8]
    for i, bad in ((8, 90001), (10, 0), (10, 257), (11, 0), (11, 1025), (12, 0), (12, 9), (3, 29), (8, 5)):
        args = list(good)
        args[i] = bad
        assert h.egtr_oi_select_f32(*args) == -1, (i, bad)
    args = list(good)
    args[14] = None
    assert h.egtr_oi_select_f32(*args) == -1
    # (stream, sop, count, B, topk, boxes, classes, N, R, gt_rels, rel_off, T, gt_boxes, gt_classes, box_off, G, ks, nk,
    #  tp, slab, acc)
    good = [None, 8, 8, 1, 100, 8, 8, 2, 30, 8, 8, 1, 8, 8, 8, 2, ks, 2, 8, 8, None]
    for i, bad in ((4, 0), (4, 1025), (7, 0), (8, 257), (17, 0), (17, 9), (11, -1), (15, -1)):
        args = list(good)
        args[i] = bad
        assert h.egtr_oi_match_f32(*args) == -1, (i, bad)
    args = list(good)
    args[16] = (ctypes.c_int * 2)(5, 1)   # not ascending
    assert h.egtr_oi_match_f32(*args) == -1
    assert h.egtr_oi_ap_f64(None, 8, 8, 8, 10, 0, 8, 8) == -1
    assert h.egtr_oi_ap_f64(None, None, 8, 8, 10, 30, 8, 8) == -1


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
        cands, targets = recorded(g)
        sl = slice(0, 8) if rank == 0 else slice(8, None)
        ev = run(cands[sl], targets[sl])
        ev.all_gather()
        q.put((rank, ev.acc.numpy(), [x.numpy() for x in ev._records()], ev.compute()))
    finally:
        dist.destroy_process_group()


def test_all_gather_two_ranks_gloo(g):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, os.path.join(HERE, "golden", "oi_eval.npz"), q))
             for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r, rest) for r, *rest in (q.get(timeout=180) for _ in procs))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    cands, targets = recorded(g)
    a = run(cands[:8], targets[:8])
    a.merge(run(cands[8:], targets[8:]))
    for r in (0, 1):
        acc, recs, metrics = got[r]
        assert np.array_equal(acc, a.acc.numpy())
        for x, y in zip(recs, a._records()):
            assert np.array_equal(x, y.numpy())
        assert metrics == a.compute()
    one = run(cands, targets)
    for k, v in one.compute().items():
        assert got[0][2][k] == pytest.approx(v, rel=1e-14, abs=1e-15), k
