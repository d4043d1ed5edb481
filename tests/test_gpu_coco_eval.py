"""GPU: COCO box-detection metrics on the device (csrc/coco_eval.hip) -- the same records, GT counts and precision /
recall tables as the host path at the configs[1] shape, no synchronisation inside update, evaluate(coco=True), and the
DeformableDetrForObjectDetection outputs through post_process."""
import json
import os
import sys
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import helpers as Hh  # noqa: E402

from egtr_amd.evaluation import COCO_STATS, CocoDetectionMetrics, coco_gt_entry, evaluate  # noqa: E402
from egtr_amd.feature_extraction import DeformableDetrFeatureExtractor  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
K = 150


def synthetic(n, seed, Q=200):
    """post_process output (100 detections per image, 150 classes; labels up to K: the no-object column) on the device,
    and explicit COCO GT dicts near some of the predicted boxes (crowd GTs and area-ignored ones included)."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(n, Q, K + 1, generator=g) - 2.0
    cxcy = torch.rand(n, Q, 2, generator=g) * 0.8 + 0.1
    wh = torch.rand(n, Q, 2, generator=g) * 0.3 + 0.01
    sizes = torch.stack([torch.randint(300, 800, (n,), generator=g), torch.randint(400, 1000, (n,), generator=g)], 1)
    gts = []
    for i in range(n):
        G = int(torch.randint(0, 25, (1,), generator=g))
        q = torch.randperm(Q, generator=g)[:G]
        lab = torch.randint(0, K, (G,), generator=g)
        logits[i, q, lab] += 5.0 * torch.rand(G, generator=g)
        h, w = float(sizes[i, 0]), float(sizes[i, 1])
        c, s = cxcy[i, q], wh[i, q]
        jit = 1.0 + 0.1 * torch.randn(G, 4, generator=g)
        box = torch.stack([(c[:, 0] - s[:, 0] / 2) * w * jit[:, 0], (c[:, 1] - s[:, 1] / 2) * h * jit[:, 1],
                           s[:, 0] * w * jit[:, 2], s[:, 1] * h * jit[:, 3]], 1).double()
        area = box[:, 2] * box[:, 3]
        odd = torch.rand(G, generator=g) < 0.2
        area = torch.where(odd, area * 4.0, area)
        crowd = (torch.rand(G, generator=g) < 0.1).to(torch.uint8)
        gts.append({"boxes": box, "area": area, "iscrowd": crowd, "labels": lab})
    out = types.SimpleNamespace(logits=logits.to(DEV), pred_boxes=torch.cat([cxcy, wh], -1).to(DEV))
    results = DeformableDetrFeatureExtractor().post_process(out, sizes.to(DEV))
    return results, gts


def host_copy(results):
    return [{k: v.cpu() for k, v in r.items()} for r in results]


def check_device_equals_host(results, gts, bs, num_classes=K):
    ev_d, ev_h = CocoDetectionMetrics(num_classes), CocoDetectionMetrics(num_classes)
    host = host_copy(results)
    for i in range(0, len(results), bs):
        ev_d.update(results[i:i + bs], gts[i:i + bs])
        ev_h.update(host[i:i + bs], gts[i:i + bs])
        for key in ("label", "rank", "match", "ignore"):
            assert torch.equal(ev_d.last_matches[key].cpu(), ev_h.last_matches[key]), key
    assert ev_d.npig.device.type == "cuda"
    assert torch.equal(ev_d.npig.cpu(), ev_h.npig)
    assert torch.equal(ev_d.precision.cpu(), ev_h.precision)
    assert torch.equal(ev_d.recall.cpu(), ev_h.recall)
    got, want = ev_d.compute(), ev_h.compute()
    assert list(got) == list(COCO_STATS)
    for k in COCO_STATS:
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
    return ev_d, got


@pytest.mark.parametrize("bs", [1, 4, 16])
def test_device_equals_host_at_config1_shape(bs):
    results, gts = synthetic(240, seed=11)
    ev, got = check_device_equals_host(results, gts, bs)
    assert ev.n_images == 240
    assert 0.0 < got["AP50"] < 1.0 and (ev.last_matches["rank"] >= 0).any()


def test_update_does_not_synchronise():
    results, gts = synthetic(24, seed=5)
    ev = CocoDetectionMetrics(K)
    ev.update(results[:2], gts[:2])        # first call: pinned staging buffer allocated outside the checked region
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(2, 24, 2):
            ev.update(results[i:i + 2], gts[i:i + 2])
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert ev.n_images == 24


def test_evaluate_coco_small_model_matches_host_path(golden_dir):
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
    host_out = {k: out[k].detach().cpu() for k in ("logits", "pred_boxes", "pred_rel")}
    targets = []
    for b in range(2):
        n = 6
        rel = torch.zeros(n, n, Rr)
        for i in range(n):
            rel[i, (i + 1) % n, (i * 3) % Rr] = 1
        targets.append({"class_labels": host_out["logits"][b, :n, :C].argmax(-1), "boxes": host_out["pred_boxes"][b, :n],
                        "rel": rel, "orig_size": sizes[b]})
    batches = [{"pixel_values": pv, "pixel_mask": pm, "labels": targets}] * 2
    got = evaluate(model, batches, C, Rr, single=True, multiple=False, max_topk=100, graphed=True, coco=True)
    vg = evaluate(model, batches, C, Rr, single=True, multiple=False, max_topk=100, graphed=True)
    assert set(got) == set(vg) | {"AP50"}
    for k, v in vg.items():
        assert got[k] == v, k
    res = DeformableDetrFeatureExtractor().post_process(
        types.SimpleNamespace(logits=out["logits"], pred_boxes=out["pred_boxes"]), sizes.to(DEV))
    ev = CocoDetectionMetrics(C)
    for _ in range(2):
        ev.update(host_copy(res), targets)
    assert abs(got["AP50"] - ev.compute()["AP50"]) <= 1e-12
    assert ev.compute()["AP50"] > 0.0


def test_object_detection_outputs_device_equals_host(golden_dir):
    g = Hh.load_golden(golden_dir, "det_small.npz")
    cfg_dict, shapes = json.loads(str(g["plain_cfg"])), json.loads(str(g["plain_shapes"]))
    seed = int(g["plain_seed"])
    model, cfg, sd = Hh.build_product_detector(cfg_dict, shapes, seed)
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    pv, pm = Hh.det_inputs(g, seed)
    with torch.no_grad():
        out = model(pixel_values=pv.to(DEV), pixel_mask=pm.to(DEV))
    sizes = torch.tensor([[480, 640], [300, 500]], device=DEV)
    results = DeformableDetrFeatureExtractor().post_process(out, sizes)
    # targets: the first queries' predicted boxes and classes as normalised GT, the way the dataset carries them
    targets = []
    for b in range(2):
        n = 5
        targets.append({"class_labels": out.logits[b, :n].argmax(-1).cpu(), "boxes": out.pred_boxes[b, :n].cpu(),
                        "orig_size": sizes[b].cpu(), "iscrowd": torch.tensor([0, 0, 0, 0, 1])})
    gts = [coco_gt_entry(t) for t in targets]
    _, got = check_device_equals_host(results, gts, 2, num_classes=cfg.num_labels)
    assert got["AP"] > 0.0
