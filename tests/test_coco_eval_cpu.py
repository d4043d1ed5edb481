"""CPU: COCO box-detection metrics' host path (egtr_amd.evaluation.CocoDetectionMetrics): hand-derived cases, the
vectorised host path against the literal restatement of COCOeval (coco_eval_restated.py) bit for bit, merge and
batching."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import coco_eval_restated as CR  # noqa: E402

from egtr_amd.evaluation import COCO_STATS, CocoDetectionMetrics, coco_gt_entry  # noqa: E402


def as_inputs(images, device="cpu"):
    """(results, gts) of restatement-style images for CocoDetectionMetrics.update."""
    results, gts = [], []
    for dets, gt in images:
        results.append({"scores": torch.tensor([d[0] for d in dets], dtype=torch.float32, device=device),
                        "labels": torch.tensor([d[1] for d in dets], dtype=torch.long, device=device),
                        "boxes": torch.tensor([list(d[2]) for d in dets], dtype=torch.float32,
                                              device=device).reshape(-1, 4)})
        gts.append({"boxes": torch.tensor([list(g[0]) for g in gt], dtype=torch.float64).reshape(-1, 4),
                    "area": torch.tensor([g[1] for g in gt], dtype=torch.float64),
                    "iscrowd": torch.tensor([g[2] for g in gt], dtype=torch.uint8),
                    "labels": torch.tensor([g[3] for g in gt], dtype=torch.long)})
    return results, gts


def run(images, K, batch=4, device="cpu"):
    ev = CocoDetectionMetrics(K)
    results, gts = as_inputs(images, device)
    for i in range(0, len(images), batch):
        ev.update(results[i:i + batch], gts[i:i + batch])
    return ev


def stats(images, K, **kw):
    return run(images, K, **kw).compute()


def close(a, b):
    """pr = tp / (fp + tp + eps): a perfect precision is 1 - 2^-52, as in COCOeval"""
    return abs(a - b) <= 1e-12


def gt(x, y, w, h, label=0, crowd=0, area=None):
    return ((float(x), float(y), float(w), float(h)), float(w * h if area is None else area), crowd, label)


# ---- hand-derived -----------------------------------------------------------------------------------------------------
def test_one_exact_detection_scores_one():
    s = stats([([(0.9, 0, (10, 10, 20, 20))], [gt(10, 10, 10, 10)])], 1)
    for k in ("AP", "AP50", "AP75", "APs", "AR1", "AR10", "AR100", "ARs"):
        assert close(s[k], 1.0), k
    for k in ("APm", "APl", "ARm", "ARl"):      # area 100 is small only: no GT in those ranges
        assert s[k] == -1.0, k


def test_iou_exactly_075():
    # detection 4 x 1 against GT 3 x 1: IoU 3 / 4, a match at the six thresholds 0.50 .. 0.75
    s = stats([([(0.9, 0, (0, 0, 4, 1))], [gt(0, 0, 3, 1)])], 1)
    assert close(s["AP50"], 1.0) and close(s["AP75"], 1.0)
    assert close(s["AP"], 0.6) and close(s["AR100"], 0.6)


def test_iou_exactly_05_matches_at_05_only():
    ev = run([([(0.9, 0, (0, 0, 2, 1))], [gt(0, 0, 1, 1)])], 1)
    s = ev.compute()
    assert close(s["AP50"], 1.0) and s["AP75"] == 0.0
    assert close(s["AP"], 0.1)
    assert ev.last_matches["match"][0, 0] == 0xF       # bits t * 4 + a: t = 0, every area range


def test_false_positive_ahead_of_true_positive():
    s = stats([([(0.9, 0, (100, 100, 110, 110)), (0.8, 0, (0, 0, 10, 10))], [gt(0, 0, 10, 10)])], 1)
    assert close(s["AP50"], 0.5) and close(s["AP"], 0.5) and s["AR100"] == 1.0 and s["AR1"] == 0.0


def test_category_with_gt_and_no_detection_scores_zero():
    ev = run([([(0.9, 0, (0, 0, 10, 10))], [gt(0, 0, 10, 10), gt(50, 50, 10, 10, label=1)])], 2)
    s = ev.compute()
    assert close(s["AP50"], 0.5)
    pc = ev.per_class()
    assert close(pc[0]["AP50"], 1.0) and pc[1]["AP50"] == 0.0 and pc[1]["AR100"] == 0.0


def test_category_without_gt_is_left_out():
    ev = run([([(0.9, 0, (0, 0, 10, 10)), (0.95, 1, (0, 0, 10, 10))], [gt(0, 0, 10, 10)])], 2)
    s = ev.compute()
    assert close(s["AP50"], 1.0) and close(s["AP"], 1.0)
    assert ev.per_class()[1]["AP50"] == -1.0
    assert (ev.precision[:, :, 1] == -1).all() and (ev.recall[:, 1] == -1).all()


def test_area_bounds_belong_to_two_ranges():
    images = [([(0.9, 0, (0, 0, 32, 32)), (0.9, 1, (0, 0, 96, 96))], [gt(0, 0, 32, 32), gt(0, 0, 96, 96, label=1)])]
    ev = run(images, 2)
    r = ev.recall[0, :, :, 2]                        # [K, A]: all, small, medium, large
    assert r.tolist() == [[1.0, 1.0, 1.0, -1.0], [1.0, -1.0, 1.0, 1.0]]
    s = ev.compute()
    assert close(s["APs"], 1.0) and close(s["APm"], 1.0) and close(s["APl"], 1.0)


def test_crowd_gt_absorbs_detections_and_is_ignored():
    # two detections inside one crowd region: both match it (ignored), nothing counts; the plain GT gives AP 1
    images = [([(0.9, 0, (0, 0, 10, 10)), (0.8, 0, (100, 100, 110, 110)), (0.7, 0, (105, 105, 115, 115))],
               [gt(0, 0, 10, 10), gt(90, 90, 40, 40, crowd=1)])]
    ev = run(images, 1)
    assert close(ev.compute()["AP"], 1.0)
    m = ev.last_matches
    assert int(m["match"][0, 1]) == int(m["match"][0, 2]) == (1 << 40) - 1
    assert int(m["ignore"][0, 1]) == int(m["ignore"][0, 2]) == (1 << 40) - 1
    assert int(ev.npig[0, 0]) == 1


# ---- host path against the restatement --------------------------------------------------------------------------------
def random_images(seed, n=40, K=6):
    rng = np.random.default_rng(seed)
    images = []
    for i in range(n):
        ng = 0 if i % 9 == 4 else int(rng.integers(0, 9))
        gts = []
        for _ in range(ng):
            side = float(rng.choice([8.0, 20.0, 32.0, 50.0, 96.0, 150.0]))
            w, h = side * float(rng.uniform(0.7, 1.3)), side * float(rng.uniform(0.7, 1.3))
            x, y = float(rng.uniform(0, 300)), float(rng.uniform(0, 300))
            crowd = int(rng.random() < 0.15)
            if crowd:
                w, h = w * 3, h * 3
            area = w * h if rng.random() < 0.7 else float(rng.choice([32.0 ** 2, 96.0 ** 2, w * h * 0.5, w * h * 3]))
            gts.append(((x, y, w, h), area, crowd, int(rng.integers(0, K))))
        nd = 0 if i % 11 == 7 else int(rng.integers(0, 30))
        dets = []
        for _ in range(nd):
            score = float(np.float32(np.round(rng.random() * 6) / 6))            # many equal scores
            if gts and rng.random() < 0.7:
                g = gts[int(rng.integers(0, len(gts)))]
                (x, y, w, h) = g[0]
                j = rng.normal(0, 0.15, 4) * np.array([w, h, w, h])
                box = (x + j[0], y + j[1], x + w + j[2], y + h + j[3])
                label = g[3] if rng.random() < 0.85 else int(rng.integers(-1, K + 2))
            else:
                x, y = rng.uniform(0, 300, 2)
                box = (x, y, x + rng.uniform(0, 120), y + rng.uniform(0, 120))
                label = int(rng.integers(-1, K + 2))
            if rng.random() < 0.05:
                box = (box[0], box[1], box[0], box[3])                              # zero width
            dets.append((score, label, tuple(float(np.float32(v)) for v in box)))
        images.append((dets, gts))
    # more than 100 detections of one category in one image, with ties
    g0 = ((10.0, 10.0, 40.0, 40.0), 1600.0, 0, 0)
    many = [(float(np.float32(0.5 + (k % 7) / 20)), 0, (float(10 + k % 5), 10.0, float(50 + k % 3), 50.0))
            for k in range(130)]
    images.append((many, [g0, ((12.0, 12.0, 40.0, 40.0), 1600.0, 0, 0)]))
    return images


def check_host_equals_restatement(images, K, batch):
    ev = run(images, K, batch=batch)
    p, r, _ = CR.evaluate(images, K)
    assert torch.equal(ev.precision, torch.from_numpy(p))
    assert torch.equal(ev.recall, torch.from_numpy(r))
    want = CR.summarize(p, r)
    got = ev.compute()
    assert list(got) == list(COCO_STATS)
    for k, v in zip(COCO_STATS, want):
        assert abs(got[k] - v) <= 1e-12, (k, got[k], v)
    return ev


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_host_path_equals_restatement(seed):
    check_host_equals_restatement(random_images(seed), 6, batch=4)


def test_batch_size_and_merge_do_not_change_results():
    images = random_images(5, n=32)
    evs = [run(images, 6, batch=bs) for bs in (1, 4, 16)]
    for e in evs[1:]:
        assert torch.equal(e.precision, evs[0].precision) and torch.equal(e.recall, evs[0].recall)
        assert torch.equal(e.npig, evs[0].npig)
        assert e.compute() == evs[0].compute()
    a, b = run(images[:13], 6), run(images[13:], 6)
    a.merge(b)
    assert a.n_images == len(images)
    assert torch.equal(a.precision, evs[0].precision) and torch.equal(a.recall, evs[0].recall)
    assert a.compute() == evs[0].compute()


def test_target_dicts_through_coco_gt_entry():
    # normalised cxcywh targets with area / size: boxes and areas rebuilt in original-image pixels
    t = {"class_labels": torch.tensor([1, 0]), "boxes": torch.tensor([[0.5, 0.5, 0.2, 0.4], [0.25, 0.25, 0.1, 0.1]]),
         "orig_size": torch.tensor([400, 600]), "size": torch.tensor([800, 1200]), "area": torch.tensor([4.0, 8.0]),
         "iscrowd": torch.tensor([0, 1])}
    e = coco_gt_entry(t)
    assert torch.allclose(e["boxes"], torch.tensor([[240.0, 120.0, 120.0, 160.0], [120.0, 80.0, 60.0, 40.0]],
                                                   dtype=torch.float64))
    assert e["area"].tolist() == [1.0, 2.0] and e["iscrowd"].tolist() == [0, 1] and e["labels"].tolist() == [1, 0]
    ev = CocoDetectionMetrics(2)
    ev.update([{"scores": torch.tensor([0.9]), "labels": torch.tensor([1]),
                "boxes": torch.tensor([[240.0, 120.0, 360.0, 280.0]])}], [t])
    assert close(ev.compute()["AP"], 1.0)


def test_argument_checks():
    with pytest.raises(ValueError):
        CocoDetectionMetrics(0)
    ev = CocoDetectionMetrics(2)
    with pytest.raises(ValueError):
        ev.update([{"scores": torch.zeros(1), "labels": torch.zeros(1, dtype=torch.long), "boxes": torch.zeros(1, 4)}],
                  [{"boxes": torch.zeros(1, 4), "labels": torch.tensor([2])}])
    empty = CocoDetectionMetrics(3).compute()
    assert all(v == -1.0 for v in empty.values())
