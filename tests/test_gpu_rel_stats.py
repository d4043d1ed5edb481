"""GPU: egtr_rel_stats_i64 / egtr_rel_seen_bits_i64 (csrc/rel_stats.hip) and egtr_sgg_zero_shot_f64 (csrc/sgg_eval.hip)
against what the reference recorded (tests/golden/rel_stats.npz): counts torch.equal at every batching, per-image zR@k rows
bit-equal in both modes, zs_acc identical across batch sizes, evaluate() on the small model."""
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
import rel_stats_inputs as RI  # noqa: E402

from egtr_amd.evaluation import SceneGraphRecall, evaluate  # noqa: E402
from egtr_amd.runtime import triplet_candidates  # noqa: E402
from egtr_amd.statistics import RelationStatistics  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KS = (20, 50, 100)


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "rel_stats.npz"))


@pytest.fixture(scope="module")
def split():
    return RI.test_split()


@pytest.fixture(scope="module")
def stats(g):
    st = RelationStatistics(RI.C, RI.R, device=DEV)
    st.update(RI.train_targets())
    assert np.array_equal(st.fg_matrix(), g["fg_vg"])
    return st


def on_device(t):
    return {k: v.to(DEV) for k, v in t.items()}


@pytest.mark.parametrize("bs", [RI.N_TRAIN, 1, 3, 7])
@pytest.mark.parametrize("where", ["host", "device"])
def test_counts_equal_the_reference(g, bs, where):
    targets = RI.train_targets()
    if where == "device":
        targets = [on_device(t) for t in targets]
    st = RelationStatistics(RI.C, RI.R, device=DEV)
    for i in range(0, len(targets), bs):
        st.update(targets[i:i + bs])
    assert st.counts.device == DEV and torch.equal(st.counts.cpu(), torch.from_numpy(g["fg_vg"]))
    fg = st.fg_matrix()
    assert fg.dtype == np.int64 and np.array_equal(fg, g["fg_oi"])


def test_dense_rel_on_device(g):
    targets = [t for t in RI.train_targets() if len(torch.unique(t["rel_triplets"], dim=0)) == len(t["rel_triplets"])]
    want = RelationStatistics(RI.C, RI.R)
    want.update(targets)
    dense = []
    for t in targets:
        rel = torch.zeros(10, 10, RI.R)
        r = t["rel_triplets"]
        rel[r[:, 0], r[:, 1], r[:, 2]] = 1.0
        dense.append({"class_labels": t["class_labels"], "rel": rel})
    st = RelationStatistics(RI.C, RI.R, device=DEV)
    st.update(dense)
    assert np.array_equal(st.fg_matrix(), want.fg_matrix())


def test_update_does_not_synchronise(g):
    targets = RI.train_targets()
    st = RelationStatistics(RI.C, RI.R, device=DEV)
    st.update(targets[:4])        # first call: the pinned buffers are allocated outside the checked region
    st.update(targets[4:8])
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(8, RI.N_TRAIN, 4):
            st.update(targets[i:i + 4])
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert np.array_equal(st.fg_matrix(), g["fg_vg"])


def test_seen_bits_on_device(g, stats):
    bits = stats.seen_bits()
    host = RelationStatistics(RI.C, RI.R)
    host.update(RI.train_targets())
    assert bits.device == DEV and torch.equal(bits.cpu(), host.seen_bits())


@pytest.mark.parametrize("where", ["host", "device"])
def test_bad_row_is_skipped_and_reported(where):
    """One image without an object, one without a relation, and a bad row in the middle of the batch: its neighbours are
    counted, it is not, and fg_matrix() raises."""
    bad_rows = torch.tensor([[0, 1, 2], [1, 3, 0], [2, 0, 1], [0, 2, RI.R], [-1, 0, 0], [1, 0, 4]])
    targets = [{"class_labels": torch.tensor([4, 5]), "rel_triplets": torch.tensor([[0, 1, 0], [1, 0, 3]])},
               {"class_labels": torch.zeros(0, dtype=torch.int64), "rel_triplets": torch.zeros(0, 3, dtype=torch.int64)},
               {"class_labels": torch.tensor([0, 1, 2]), "rel_triplets": bad_rows},
               {"class_labels": torch.tensor([3, 3]), "rel_triplets": torch.zeros(0, 3, dtype=torch.int64)},
               {"class_labels": torch.tensor([6, RI.C + 1, 2]), "rel_triplets": torch.tensor([[0, 2, 1], [0, 1, 1], [2, 0, 2]])}]
    if where == "device":
        targets = [on_device(t) for t in targets]
    st = RelationStatistics(RI.C, RI.R, device=DEV)
    st.update(targets)
    want = torch.zeros(RI.C + 1, RI.C + 1, RI.R, dtype=torch.int64)
    for cs, co, p in ((4, 5, 0), (5, 4, 3), (0, 1, 2), (2, 0, 1), (1, 0, 4), (6, 2, 1), (2, 6, 2)):
        want[cs, co, p] += 1
    assert torch.equal(st.counts.cpu(), want)
    with pytest.raises(ValueError):
        st.fg_matrix()
    with pytest.raises(ValueError):
        st.finalize()
    clean = RelationStatistics(RI.C, RI.R, device=DEV)
    clean.update(targets[:2] + targets[3:4])
    assert clean.fg_matrix().sum() == 2


def evaluator(mode, train_counts, **kw):
    return SceneGraphRecall(RI.R, multiple_preds=(mode == "m"), train_counts=train_counts, **kw)


def run(ev, cands, targets, bs=RI.N_TEST):
    for i in range(0, len(cands), bs):
        ev.update(cands[i:i + bs], targets[i:i + bs])
    return ev


@pytest.mark.parametrize("top,prefix", [(None, ""), (10, "k10_")])
@pytest.mark.parametrize("mode", ["m", "s"])
def test_device_zero_shot_matches_reference(g, split, stats, mode, top, prefix):
    cands, targets, _ = split
    c = RI.candidates(cands, mode, device=DEV, top=top)
    accs = []
    for bs in (1, 5, RI.N_TEST):
        ev = run(evaluator(mode, stats, keep_per_image=True), c, targets, bs=bs)
        assert ev.zs_acc.device == DEV
        assert np.array_equal(ev.per_image_zero_shot().numpy(), g[f"{prefix}{mode}_zs_recall"])     # bit-equal rows
        accs.append(ev.zs_acc.cpu())
    assert torch.equal(accs[0], accs[1]) and torch.equal(accs[0], accs[2])
    got = ev.zero_shot()
    for j, k in enumerate(KS):
        assert abs(got[f"zR@{k}"] - g[f"{prefix}{mode}_zs_stats"][j]) <= 1e-12
    nz = g["n_zero_shot"]
    assert ev.n_zero_shot_images == int((nz > 0).sum()) and ev.n_zero_shot_triplets == int(nz.sum())
    # the host twin computes the same state
    host = run(evaluator(mode, g["fg_vg"]), RI.candidates(cands, mode, top=top), targets)
    assert torch.equal(host.zs_acc, accs[0])


@pytest.mark.parametrize("mode", ["m", "s"])
def test_ordinary_metrics_unchanged_by_train_counts(g, split, stats, mode):
    cands, targets, _ = split
    c = RI.candidates(cands, mode, device=DEV)
    plain = run(SceneGraphRecall(RI.R, multiple_preds=(mode == "m"), keep_per_image=True), c, targets, bs=5)
    for tc, kw in ((stats, {}), (g["fg_vg"], {}), (stats.seen_bits(), {"train_num_labels": RI.C})):
        ev = run(evaluator(mode, tc, keep_per_image=True, **kw), c, targets, bs=5)
        assert ev.width == plain.width and torch.equal(ev.acc, plain.acc)
        assert ev.compute() == plain.compute() and ev.mean_recall() == plain.mean_recall()
        assert torch.equal(ev.per_image(), plain.per_image())
    assert np.array_equal(plain.per_image().numpy(), g[f"{mode}_recall"])
    assert plain.zs_acc is None


def test_no_zero_shot_triplet_leaves_zs_acc_at_zero(g, split, stats):
    cands, targets, _ = split
    idx = [i for i, n in enumerate(g["n_zero_shot"]) if n == 0]
    c = RI.candidates(cands, "s", device=DEV)
    ev = evaluator("s", stats)
    ev.update([c[i] for i in idx], [targets[i] for i in idx])
    assert ev.n_images == len(idx) and not ev.zs_acc.any()
    assert all(math.isnan(v) for v in ev.zero_shot().values())


def test_zero_shot_update_does_not_synchronise(g, split, stats):
    cands, targets, _ = split
    c = RI.candidates(cands, "m", device=DEV)
    ev = evaluator("m", stats)
    ev.update(c[:2], targets[:2])
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(2, RI.N_TEST, 2):
            ev.update(c[i:i + 2], targets[i:i + 2])
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert abs(ev.zero_shot()["zR@100"] - g["m_zs_stats"][2]) <= 1e-12


def test_evaluate_adds_zero_shot_keys(golden_dir):
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
    logits, boxes, pred_rel = out["logits"].cpu(), out["pred_boxes"].cpu(), out["pred_rel"].cpu()
    sizes = torch.tensor([[480, 640], [300, 500]])
    targets = []
    for b in range(2):       # targets from the model's own predictions, as in test_gpu_sgg_eval.py
        n = 6
        rows = sorted({(i, (i + 1) % n, (i * 3) % R) for i in range(n)}
                      | {(i, (i + 2) % n, int(pred_rel[b, i, (i + 2) % n].argmax())) for i in range(n)})
        targets.append({"class_labels": logits[b, :n, :C].argmax(-1), "boxes": boxes[b, :n],
                        "rel_triplets": torch.tensor(rows, dtype=torch.int64), "orig_size": sizes[b]})
    train = RelationStatistics(C, R)      # "training set": every second row of the first image
    train.update([dict(targets[0], rel_triplets=targets[0]["rel_triplets"][::2])])
    batches = [{"pixel_values": pv, "pixel_mask": pm, "labels": targets}] * 2
    plain = evaluate(model, batches, C, R, single=True, multiple=True, max_topk=100, graphed=False)
    got = evaluate(model, batches, C, R, single=True, multiple=True, max_topk=100, graphed=False, train_counts=train)
    zs_keys = {f"{p}zR@{k}" for p in ("", "(single)") for k in KS}
    assert set(got) == set(plain) | zs_keys and not set(plain) & zs_keys
    for k, v in plain.items():
        assert got[k] == v, (k, got[k], v)
    # the zero-shot numbers against the host twin on the same (host) outputs, within the tolerance of the existing
    # evaluate() test: the device chain's scores differ from the host's in the last bits
    host_out = {k: out[k].detach().cpu() for k in ("logits", "pred_boxes", "pred_rel", "pred_connectivity")
                if k in out and out[k] is not None}
    for mode, key in (("multiple", ""), ("single", "(single)")):
        ev = SceneGraphRecall(R, multiple_preds=(mode == "multiple"), train_counts=train)
        for _ in range(2):
            ev.update(triplet_candidates(host_out, C, sizes, 100, mode=mode), targets)
        assert ev.n_zero_shot_triplets > 0
        for k, v in ev.zero_shot().items():
            assert abs(got[key + k] - v) <= 1e-12, (key + k, got[key + k], v)
