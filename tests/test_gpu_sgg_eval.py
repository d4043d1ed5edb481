"""GPU: the scene-graph evaluator kernel (csrc/sgg_eval.hip, egtr_sgg_eval_f32) and the device path of
egtr_amd.evaluation -- first ranks equal to the host matching, per-image recalls bit-equal to the reference's recorded
evaluators (tests/golden/sgg_eval.npz), the device chain triplet_candidates -> evaluator, batch-size independence, no
synchronisation inside update, evaluate() on the small model."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import helpers as Hh  # noqa: E402
import sgg_eval_inputs as SI  # noqa: E402

from egtr_amd import _lib  # noqa: E402
from egtr_amd.evaluation import (SceneGraphRecall, _bbox_iou_pyx, evaluate, first_ranks_host, gt_entry,  # noqa: E402
                                 numpy_argmax)
from egtr_amd.runtime import triplet_candidates  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KS = (20, 50, 100)


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "sgg_eval.npz"))


def recorded(g, mode, prefix="", device=DEV):
    _, targets, _ = SI.sgg_eval_inputs(seed=int(g["seed"]), chain=bool(prefix))
    cands = []
    for j in range(len(targets)):
        cands.append({"pred_boxes": torch.from_numpy(g[f"{prefix}{j}_pred_boxes"]).to(device),
                      "pred_classes": torch.from_numpy(g[f"{prefix}{j}_pred_classes"]).to(device),
                      "pred_rel_inds": torch.from_numpy(g[f"{prefix}{mode}{j}_pred_rel_inds"]).to(device),
                      "rel_scores": torch.from_numpy(g[f"{prefix}{mode}{j}_rel_scores"]).to(device)})
    return cands, targets


def run(cands, targets, mode, bs=16, **kw):
    ev = SceneGraphRecall(SI.R, multiple_preds=(mode == "m"), **kw)
    for i in range(0, len(cands), bs):
        ev.update(cands[i:i + bs], targets[i:i + bs])
    return ev


# ---------------------------------------------------------------------------------------------------------------------
def stress_batch(seed, B, K, R, multiple, n_obj=60):
    """Random images with many label matches (3 classes), integer boxes incl. IoU exactly 0.5 / just below, up to 300 GT
    triplets, NaN and tied rows in single mode."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cands, targets = [], []
    H, Wd = 512, 1024
    for b in range(B):
        G = int(rng.integers(2, 30))
        d = rng.integers(3, 30, G)
        x0, y0 = rng.integers(0, 700, G), rng.integers(0, 300, G)
        hh = rng.integers(5, 150, G)
        gt = np.stack([x0, y0, x0 + 3 * d - 1, y0 + hh - 1], 1).astype(np.float64)
        cls = rng.integers(0, 3, G)
        T = 0 if b == 3 else int(rng.integers(1, 301))
        rel = np.zeros((G, G, R), np.float32)
        for _ in range(T):
            s, o = rng.integers(0, G, 2)
            rel[s, o, rng.integers(0, min(R, 5))] = 1
        cx, cy = (gt[:, 0] + gt[:, 2]) / 2 / Wd, (gt[:, 1] + gt[:, 3]) / 2 / H
        w, h = (gt[:, 2] - gt[:, 0]) / Wd, (gt[:, 3] - gt[:, 1]) / H
        targets.append({"class_labels": torch.from_numpy(cls), "orig_size": torch.tensor([H, Wd]),
                        "boxes": torch.from_numpy(np.stack([cx, cy, w, h], 1).astype(np.float32)),
                        "rel": torch.from_numpy(rel)})
        src = rng.integers(0, G, n_obj)
        shift = rng.integers(0, 3, n_obj)
        dx = np.where(shift == 0, 0, np.where(shift == 1, d[src], d[src] + 1))        # IoU 1, exactly 0.5, below
        pb = gt[src] + np.stack([dx, np.zeros(n_obj), dx, np.zeros(n_obj)], 1)
        pb = pb + np.where(rng.random((n_obj, 1)) < 0.2, rng.uniform(-3, 3, (n_obj, 4)), 0)
        pcls = np.where(rng.random(n_obj) < 0.8, cls[src], rng.integers(0, 3, n_obj))
        so = rng.integers(0, n_obj, (K, 2))
        c = {"pred_boxes": torch.from_numpy(pb.astype(np.float32)), "pred_classes": torch.from_numpy(pcls)}
        if multiple:
            c["pred_rel_inds"] = torch.from_numpy(np.concatenate([so, rng.integers(0, min(R, 5), (K, 1))], 1))
        else:
            sc = np.round(rng.random((K, R)) * 4).astype(np.float32) / 4
            sc[rng.random(K) < 0.05, rng.integers(0, R)] = np.nan
            c["pred_rel_inds"] = torch.from_numpy(so)
            c["rel_scores"] = torch.from_numpy(sc)
        cands.append(c)
    return cands, targets


@pytest.mark.parametrize("K,R,multiple", [(100, 50, True), (100, 50, False), (1000, 30, True), (1000, 30, False)])
def test_first_rank_equals_host_stress(K, R, multiple):
    cands, targets = stress_batch(100 + K + R + multiple, 12, K, R, multiple)
    ev = SceneGraphRecall(R, multiple_preds=multiple, keep_per_image=True)
    ev.update([{k: v.to(DEV) for k, v in c.items()} for c in cands], targets)
    got = ev.last_first_rank.cpu().long()
    want = []
    for c, t in zip(cands, targets):
        e = gt_entry(t)
        rels = c["pred_rel_inds"] if multiple else torch.cat([c["pred_rel_inds"], numpy_argmax(c["rel_scores"])[:, None]], 1)
        want.append(first_ranks_host(rels, c["pred_boxes"], c["pred_classes"], e["gt_relations"], e["gt_boxes"],
                                     e["gt_classes"]))
    want = torch.cat(want)
    assert got.shape == want.shape and want.shape[0] > 1000
    assert torch.equal(got, want)
    assert (want < K).sum() > 10    # the stress set has matches
    host = SceneGraphRecall(R, multiple_preds=multiple)
    host.update(cands, targets)
    assert torch.equal(ev.acc.cpu(), host.acc)      # same rows, same image-order fold: bit-equal
    assert ev.skipped == 1


@pytest.mark.parametrize("prefix", ["", "chain_"])
@pytest.mark.parametrize("mode", ["m", "s"])
def test_device_matches_reference_fixture(g, mode, prefix):
    cands, targets = recorded(g, mode, prefix)
    ev = run(cands, targets, mode, keep_per_image=True)
    assert np.array_equal(ev.per_image().numpy(), g[f"{prefix}{mode}_recall"])
    got, mr = ev.compute(), ev.mean_recall()
    for j, k in enumerate(KS):
        assert abs(got[f"R@{k}"] - g[f"{prefix}{mode}_stats"][j]) <= 1e-12
        assert abs(mr[f"mR@{k}"] - g[f"{prefix}{mode}_mr"][j]) <= 1e-12
    ps = g[f"{prefix}{mode}_pred_stats"]
    for p, v in ev.per_predicate().items():
        for j, k in enumerate(KS):
            assert (math.isnan(v[f"R@{k}"]) and math.isnan(ps[p, j])) or abs(v[f"R@{k}"] - ps[p, j]) <= 1e-12


@pytest.mark.parametrize("mode", ["m", "s"])
def test_chain_triplet_candidates_on_device(g, mode):
    outputs, targets, meta = SI.sgg_eval_inputs(seed=int(g["seed"]), chain=True)
    outputs = {k: v.to(DEV) for k, v in outputs.items()}
    sizes = torch.stack([t["orig_size"] for t in targets]).to(DEV)
    cands = triplet_candidates(outputs, meta["num_labels"], sizes, 100, mode="multiple" if mode == "m" else "single")
    ev = run(cands, targets, mode, bs=4, keep_per_image=True)
    assert np.array_equal(ev.per_image().numpy(), g[f"chain_{mode}_recall"])
    got, mr = ev.compute(), ev.mean_recall()
    for j, k in enumerate(KS):
        assert abs(got[f"R@{k}"] - g[f"chain_{mode}_stats"][j]) <= 1e-12
        assert abs(mr[f"mR@{k}"] - g[f"chain_{mode}_mr"][j]) <= 1e-12


@pytest.mark.parametrize("mode", ["m", "s"])
def test_batch_size_independent_on_device(g, mode):
    cands, targets = recorded(g, mode)
    accs = [run(cands, targets, mode, bs=bs).acc.cpu() for bs in (1, 4, 16)]
    assert torch.equal(accs[0], accs[1]) and torch.equal(accs[0], accs[2])


def test_update_does_not_synchronise(g):
    cands, targets = recorded(g, "s")
    ev = SceneGraphRecall(SI.R)
    ev.update(cands[:2], targets[:2])        # first call: pinned staging buffer allocated outside the checked region
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(2, 16, 2):
            ev.update(cands[i:i + 2], targets[i:i + 2])
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert ev.n_images == 16


def test_evaluate_small_model_matches_host_path(golden_dir):
    gs = Hh.load_golden(golden_dir, "sgg_small.npz")
    cfg_dict, shapes = json.loads(str(gs["cfg"])), json.loads(str(gs["shapes"]))
    model, cfg, sd = Hh.build_product_model(cfg_dict, shapes, int(gs["seed"]))
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    pv, pm = Hh.small_inputs(gs)
    with torch.no_grad():
        out = model(pixel_values=pv.to(DEV), pixel_mask=pm.to(DEV), output_attentions=False,
                    output_attention_states=True, output_hidden_states=True)
    C, R = cfg.num_labels, cfg.num_rel_labels
    # targets built from the model's own predictions (so that recalls are not all zero): the best boxes / pairs
    targets = []
    sizes = torch.tensor([[480, 640], [300, 500]])
    host_out = {k: out[k].detach().cpu() for k in ("logits", "pred_boxes", "pred_rel", "pred_connectivity")
                if k in out and out[k] is not None}
    for b in range(2):
        n = 6
        rel = torch.zeros(n, n, R)
        for i in range(n):
            rel[i, (i + 1) % n, (i * 3) % R] = 1
            rel[i, (i + 2) % n, int(host_out["pred_rel"][b, i, (i + 2) % n].argmax())] = 1
        targets.append({"class_labels": host_out["logits"][b, :n, :C].argmax(-1), "boxes": host_out["pred_boxes"][b, :n],
                        "rel": rel, "orig_size": sizes[b]})
    batches = [{"pixel_values": pv, "pixel_mask": pm, "labels": targets}] * 2
    got = evaluate(model, batches, C, R, single=True, multiple=True, max_topk=100, graphed=True)
    want = {}
    for mode, key in (("multiple", ""), ("single", "(single)")):
        ev = SceneGraphRecall(R, multiple_preds=(mode == "multiple"))
        for _ in range(2):
            ev.update(triplet_candidates(host_out, C, sizes, 100, mode=mode), targets)
        want.update({key + k: v for k, v in ev.compute().items()})
        want.update({key + k: v for k, v in ev.mean_recall().items()})
    assert set(got) == set(want) == {f"{p}{m}@{k}" for p in ("", "(single)") for m in ("R", "mR") for k in KS}
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-12, (k, got[k], v)
    assert want["(single)R@100"] > 0


def test_sgg_eval_rejects_bad_arguments():
    h = _lib.lib()
    d = torch.zeros(4096, dtype=torch.int64, device=DEV)
    p = d.data_ptr()
    slab = torch.zeros(4096, dtype=torch.float64, device=DEV)

    def call(cols=3, scores=p, K=10, N=5, R=10, ks=(20, 50), T=1, G=2, thr=0.5, B=1):
        arr = (ctypes.c_int * max(1, len(ks)))(*ks)
        return h.egtr_sgg_eval_f32(None, p, cols, scores, p, p, B, K, N, R, p, p, T, p, p, p, G, arr, len(ks), thr, None,
                                   slab.data_ptr(), None)

    assert call() == 0
    torch.cuda.synchronize()
    assert call(cols=4) == -1
    assert call(cols=2, scores=None) == -1
    assert call(K=1025) == -1
    assert call(R=257) == -1
    assert call(R=0) == -1
    assert call(ks=()) == -1
    assert call(ks=(50, 20)) == -1
    assert call(ks=tuple(range(1, 10))) == -1
    assert call(thr=float("nan")) == -1
    assert call(B=-1) == -1
    assert call(N=0) == -1
    assert h.egtr_sgg_eval_width(0, 3) == -1 and h.egtr_sgg_eval_width(50, 3) == 3 + 2 + 50 * 4


def test_bbox_overlaps_f64_unchanged_by_refactor():
    rng = np.random.Generator(np.random.PCG64(5))
    a = np.floor(rng.uniform(0, 100, (50, 4)))
    a[:, 2:] += a[:, :2]
    q = np.floor(rng.uniform(0, 100, (40, 4)))
    q[:, 2:] += q[:, :2]
    shift = (a[:10, 2] - a[:10, 0] + 1) / 3          # same boxes shifted by a third of their width: IoU 0.5 when exact
    zero = np.zeros(10)
    q[:10] = a[:10] + np.stack([shift, zero, shift, zero], 1)
    A, Q = torch.from_numpy(a).to(DEV), torch.from_numpy(q).to(DEV)
    out = torch.empty(50, 40, dtype=torch.float64, device=DEV)
    _lib.check(_lib.lib().egtr_bbox_overlaps_f64(None, A.data_ptr(), Q.data_ptr(), 50, 40, 0, out.data_ptr()), "bbox")
    want = _bbox_iou_pyx(torch.from_numpy(a)[:, None, :], torch.from_numpy(q)[None, :, :])
    assert torch.equal(out.cpu(), want)
