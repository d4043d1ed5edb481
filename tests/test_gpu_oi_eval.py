"""GPU: the Open Images relation metrics on the device (csrc/oi_eval.hip) -- the reference fixture bit for bit, the
selection against the torch composition at the configs[3] shape and where the top-`topk` boundary falls inside a tie,
between adjacent floats or beyond the survivors, no synchronisation inside update, evaluate(oi=True)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import helpers as Hh  # noqa: E402
import oi_eval_inputs as OI  # noqa: E402
from test_oi_eval_cpu import check_against_reference, check_detections, recorded, run  # noqa: E402

from egtr_amd.evaluation import OpenImagesRelationMetrics, evaluate, oi_select_host  # noqa: E402
from egtr_amd.runtime import triplet_candidates  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
R = OI.R


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "oi_eval.npz"))


def test_device_matches_reference_fixture(g):
    cands, targets = recorded(g, DEV)
    host_cands, _ = recorded(g)
    ev = OpenImagesRelationMetrics(R)
    rows = []
    for i in range(0, len(cands), 4):
        ev.update(cands[i:i + 4], targets[i:i + 4])
        sop, score, count = (x.cpu() for x in ev.last_detections)
        for b in range(sop.shape[0]):
            j, n = i + b, int(count[b])
            assert (sop[b, n:] == -1).all()
            check_detections(g, j, sop[b, :n], score[b, :n], host_cands[j]["pred_classes"],
                             host_cands[j]["pred_boxes"])
        rows.append(ev.last_rows.cpu())
    assert ev.acc.device.type == "cuda"
    check_against_reference(g, ev, torch.cat(rows))


def test_batch_size_independent_on_device(g):
    cands, targets = recorded(g, DEV)
    evs = [run(cands, targets, bs) for bs in (1, 3, 20)]
    for e in evs[1:]:
        assert torch.equal(e.acc, evs[0].acc)
        assert e.compute() == evs[0].compute()


def _random_batch(B, N, Rr, seed):
    """triplet_candidates(mode="oi")-shaped views of one [B, N, N, R] tensor, tie-free, plus random targets."""
    gen = torch.Generator().manual_seed(seed)
    rel = torch.rand(B, N, N, Rr, generator=gen)
    obj = 0.2 + 0.8 * torch.rand(B, N, generator=gen)
    cls = torch.randint(0, 6, (B, N), generator=gen)
    xy = torch.rand(B, N, 2, generator=gen) * 400
    wh = 20 + torch.rand(B, N, 2, generator=gen) * 100
    boxes = torch.cat([xy, xy + wh], -1).round()
    pairs = torch.cartesian_prod(torch.arange(N), torch.arange(N))
    targets = []
    for b in range(B):
        G = 12
        rels = torch.zeros(G, G, Rr)
        for t in range(10):
            s, o = int(torch.randint(0, G, (1,), generator=gen)), int(torch.randint(0, G, (1,), generator=gen))
            rels[s, (o if o != s else (s + 1) % G), int(torch.randint(0, Rr, (1,), generator=gen))] = 1
        bx = boxes[b, :G] + torch.randint(-3, 4, (G, 4), generator=gen).float()   # near copies of the first objects
        cxcywh = torch.stack([(bx[:, 0] + bx[:, 2]) / 2 / 1024, (bx[:, 1] + bx[:, 3]) / 2 / 512,
                              (bx[:, 2] - bx[:, 0]) / 1024, (bx[:, 3] - bx[:, 1]) / 512], -1)
        targets.append({"class_labels": cls[b, :G].clone(), "boxes": cxcywh, "rel": rels,
                        "orig_size": torch.tensor([512, 1024])})
    for b in range(B):
        OI.check_ties(rel[b].reshape(N * N, Rr).numpy(), obj[b].numpy(), pairs.numpy())
    return rel, obj, cls, boxes, pairs, targets


@pytest.mark.parametrize("B", [1, 2, 4])
def test_select_equals_torch_at_config3_shape(B):
    N, Rr = 200, 30
    rel, obj, cls, boxes, pairs, targets = _random_batch(B, N, Rr, seed=100 + B)
    d_rel, d_pairs = rel.to(DEV), pairs.to(DEV)
    cands = [{"pred_boxes": boxes[b].to(DEV), "pred_classes": cls[b].to(DEV), "obj_scores": obj[b].to(DEV),
              "sbj_obj_inds": d_pairs, "pred_scores": d_rel[b].reshape(N * N, Rr)} for b in range(B)]
    host = [{"pred_boxes": boxes[b], "pred_classes": cls[b], "obj_scores": obj[b], "sbj_obj_inds": pairs,
             "pred_scores": rel[b].reshape(N * N, Rr)} for b in range(B)]
    ev_d, ev_h = OpenImagesRelationMetrics(Rr), OpenImagesRelationMetrics(Rr)
    ev_d.update(cands, targets)
    ev_h.update(host, targets)
    sop, score, count = (x.cpu() for x in ev_d.last_detections)
    for b in range(B):
        want_sop, want_score = oi_select_host(host[b]["pred_scores"], obj[b], pairs)
        n = int(count[b])
        assert n == want_sop.shape[0] == 100
        assert torch.equal(sop[b, :n].long(), want_sop)
        assert torch.equal(score[b, :n], want_score)
    assert torch.equal(ev_d.acc.cpu(), ev_h.acc)
    for x, y in zip(ev_d._records(), ev_h._records()):
        assert torch.equal(x.cpu(), y)
    got, want = ev_d.compute(), ev_h.compute()
    assert set(got) == set(want)
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-12, (k, got[k], v)


_BN, _BR, _BKK = 24, 6, 2      # 576 pairs: two partial blocks of 512, so the merge pass sees two lists


def _boundary_scores(case):
    """pred_scores [576, 6] whose per-pair top-2 values (the pair-major [M, 2] array the selection ranks) are placed by
    ``case``; object scores are 1, so spo is the value itself."""
    M, below = _BN * _BN, np.float32(np.nextafter(np.float32(0.5), np.float32(0)))
    if case == "full_tie":                         # the whole list ties: the index half of the key decides
        return torch.full((M, _BR), 0.5)
    rng = np.random.Generator(np.random.PCG64({"adjacent": 1, "few": 2, "exact": 3}[case]))
    if case == "adjacent":                         # 100 at 0.5, 100 at the float below, the rest far below
        vals, fill = np.full(M * _BKK, 0.25, np.float32), 0.125
        pos = rng.permutation(M * _BKK)[:200]
        vals[pos[:100]], vals[pos[100:]] = 0.5, below
    else:                                          # 7 or exactly 100 survivors of the > 1e-5 cut, equal values among them
        n = 7 if case == "few" else 100
        vals, fill = np.full(M * _BKK, 1e-6, np.float32), 0.0
        vals[rng.permutation(M * _BKK)[:n]] = (0.2 + 0.7 * rng.integers(0, max(n // 2, 4), n) / n).astype(np.float32)
    vals = -np.sort(-vals.reshape(M, _BKK), axis=1)                    # a pair's best predicate comes first
    rows = np.full((M, _BR), fill, np.float32)
    for m in range(M):                                                 # equal values: the lower predicate index is first
        a, b = np.sort(rng.choice(_BR, 2, replace=False))
        if vals[m, 0] != vals[m, 1] and rng.random() < 0.5:
            a, b = b, a
        rows[m, a], rows[m, b] = vals[m, 0], vals[m, 1]
    return torch.from_numpy(rows)


@pytest.fixture(scope="module")
def boundary():
    """{case: (pred_scores, {topk: (sop, score) of oi_select_host})}: the host's stable sort defines the tie order."""
    obj = torch.ones(_BN)
    pairs = torch.cartesian_prod(torch.arange(_BN), torch.arange(_BN))
    out = {}
    for case in ("full_tie", "adjacent", "few", "exact"):
        ps = _boundary_scores(case)
        out[case] = (ps, {k: oi_select_host(ps, obj, pairs, k, _BKK) for k in (100, 101)})
    return out


def _select_on_device(score_list, topk):
    rel = torch.zeros(2, 2, _BR)
    rel[0, 1, 0] = 1
    target = {"class_labels": torch.zeros(2, dtype=torch.long), "boxes": torch.full((2, 4), 0.25), "rel": rel,
              "orig_size": torch.tensor([64, 64])}
    cands = [{"pred_boxes": torch.zeros(_BN, 4, device=DEV), "pred_classes": torch.zeros(_BN, dtype=torch.long, device=DEV),
              "obj_scores": torch.ones(_BN, device=DEV), "pred_scores": ps.to(DEV)} for ps in score_list]
    ev = OpenImagesRelationMetrics(_BR, topk=topk, prd_k=_BKK)
    ev.update(cands, [target] * len(cands))
    return [x.cpu() for x in ev.last_detections]


@pytest.mark.parametrize("case,topk", [("full_tie", 100), ("adjacent", 100), ("adjacent", 101), ("few", 100),
                                       ("exact", 100)])
def test_select_boundaries_equal_host(boundary, case, topk):
    names = list(boundary)
    other = names[(names.index(case) + 1) % len(names)]
    want = {c: boundary[c][1][topk] for c in (case, other)}
    ps = {c: boundary[c][0] for c in (case, other)}
    # the properties the cases were built for, on the host result that defines them
    w_sop, w_score = want[case]
    if case == "full_tie":
        flat = torch.arange(100)
        assert torch.equal(w_sop, torch.stack([flat // 2 // _BN, flat // 2 % _BN, flat % 2], 1)) and (w_score == 0.5).all()
    elif case == "adjacent":
        assert (w_score[:100] == 0.5).all() and w_score.shape[0] == topk
        assert topk == 100 or w_score[100] == np.nextafter(np.float32(0.5), np.float32(0))
    else:
        assert w_score.shape[0] == (7 if case == "few" else 100) and (w_score[1:] <= w_score[:-1]).all()
        assert len(torch.unique(w_score)) < w_score.shape[0]          # ties among the survivors
    # alone, and next to another image on either side: an image's selection does not depend on its neighbour
    for order in ((case,), (case, other), (other, case)):
        sop, score, count = _select_on_device([ps[c] for c in order], topk)
        for b, c in enumerate(order):
            n = want[c][0].shape[0]
            assert int(count[b]) == n, (order, b)
            assert torch.equal(sop[b, :n].long(), want[c][0]), (order, b)
            assert torch.equal(score[b, :n], want[c][1]), (order, b)
            assert (sop[b, n:] == -1).all() and (score[b, n:] == 0).all(), (order, b)


def test_shared_pairs_absent_and_stacked_inputs():
    # no sbj_obj_inds (the cartesian product) and non-view pred_scores (stacked on the device) give the same result
    N, Rr = 24, 30
    rel, obj, cls, boxes, pairs, targets = _random_batch(2, N, Rr, seed=7)
    base = [{"pred_boxes": boxes[b].to(DEV), "pred_classes": cls[b].to(DEV), "obj_scores": obj[b].to(DEV),
             "pred_scores": rel[b].reshape(N * N, Rr).to(DEV).clone()} for b in range(2)]
    with_pairs = [dict(c, sbj_obj_inds=pairs.to(DEV)) for c in base]
    a, b_ = OpenImagesRelationMetrics(Rr), OpenImagesRelationMetrics(Rr)
    a.update(base, targets)
    b_.update(with_pairs, targets)
    assert torch.equal(a.last_detections[0], b_.last_detections[0])
    assert a.compute() == b_.compute()


def test_update_does_not_synchronise(g):
    cands, targets = recorded(g, DEV)
    ev = OpenImagesRelationMetrics(R)
    ev.update(cands[:2], targets[:2])        # first call: pinned staging buffer allocated outside the checked region
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(2, 20, 2):
            ev.update(cands[i:i + 2], targets[i:i + 2])
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert ev.n_images == 20


def test_evaluate_oi_small_model_matches_host_path(golden_dir):
    gs = Hh.load_golden(golden_dir, "sgg_small.npz")
    cfg_dict, shapes = json.loads(str(gs["cfg"])), json.loads(str(gs["shapes"]))
    model, cfg, sd = Hh.build_product_model(cfg_dict, shapes, int(gs["seed"]))
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    pv, pm = Hh.small_inputs(gs)
    with torch.no_grad():
        out = model(pixel_values=pv.to(DEV), pixel_mask=pm.to(DEV), output_attentions=False,
                    output_attention_states=True, output_hidden_states=True)
    C, Rr = cfg.num_labels, cfg.num_rel_labels
    sizes = torch.tensor([[480, 640], [300, 500]])
    host_out = {k: out[k].detach().cpu() for k in ("logits", "pred_boxes", "pred_rel", "pred_connectivity")
                if k in out and out[k] is not None}
    targets = []
    for b in range(2):
        n = 6
        rel = torch.zeros(n, n, Rr)
        for i in range(n):
            rel[i, (i + 1) % n, (i * 3) % Rr] = 1
            rel[i, (i + 2) % n, int(host_out["pred_rel"][b, i, (i + 2) % n].argmax())] = 1
        targets.append({"class_labels": host_out["logits"][b, :n, :C].argmax(-1), "boxes": host_out["pred_boxes"][b, :n],
                        "rel": rel, "orig_size": sizes[b]})
    batches = [{"pixel_values": pv, "pixel_mask": pm, "labels": targets}] * 2
    got = evaluate(model, batches, C, Rr, single=True, multiple=False, max_topk=100, graphed=True, oi=True)
    vg = evaluate(model, batches, C, Rr, single=True, multiple=False, max_topk=100, graphed=True)
    ev = OpenImagesRelationMetrics(Rr)
    for _ in range(2):
        ev.update(triplet_candidates(host_out, C, sizes, 100, mode="oi"), targets)
    want = {(f"(oi){k}" if k.startswith("R@") else k): v for k, v in ev.compute().items()}
    assert set(got) == set(vg) | set(want)
    for k, v in vg.items():
        assert got[k] == v, k
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-12, (k, got[k], v)
