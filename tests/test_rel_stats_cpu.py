"""CPU: RelationStatistics and the zero-shot recall of SceneGraphRecall on the host, against what the reference's own
vg_get_statistics / oi_get_statistics and BasicSceneGraphEvaluator recorded (tests/golden/rel_stats.npz,
make_golden_rel_stats.py): the count matrix array_equal, per-image zR@k rows bit-equal, aggregates within the 1e-12 that
test_sgg_eval_cpu.py uses for the left fold against np.mean."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import rel_stats_inputs as RI  # noqa: E402

from egtr_amd.evaluation import SceneGraphRecall, seen_bits_host  # noqa: E402
from egtr_amd.statistics import RelationStatistics  # noqa: E402

KS = (20, 50, 100)


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "rel_stats.npz"))


@pytest.fixture(scope="module")
def split():
    return RI.test_split()


def whole(targets=None):
    st = RelationStatistics(RI.C, RI.R)
    st.update(RI.train_targets() if targets is None else targets)
    return st


def dense(t, n=10):
    rel = torch.zeros(n, n, RI.R)
    r = t["rel_triplets"]
    rel[r[:, 0], r[:, 1], r[:, 2]] = 1.0
    return {"class_labels": t["class_labels"], "rel": rel}


def test_fixture_is_the_seeded_split(g):
    assert int(g["seed"]) == RI.SEED
    assert np.array_equal(g["fg_vg"], RI.count(RI.train_split()))


def test_counts_equal_both_reference_matrices(g):
    fg = whole().fg_matrix()
    assert fg.dtype == np.int64 and fg.shape == (RI.C + 1, RI.C + 1, RI.R)
    assert np.array_equal(fg, g["fg_vg"]) and np.array_equal(fg, g["fg_oi"])
    one_by_one = RelationStatistics(RI.C, RI.R)
    for t in RI.train_targets():
        one_by_one.update([t])
    assert np.array_equal(one_by_one.fg_matrix(), g["fg_vg"])


def test_dense_rel_counts_each_nonzero_entry(g):
    """Dense targets cannot hold a duplicate: on the images without one they give the reference's counts of those images."""
    targets = [t for t in RI.train_targets() if len(torch.unique(t["rel_triplets"], dim=0)) == len(t["rel_triplets"])]
    assert 5 < len(targets) < RI.N_TRAIN
    split = [(t["class_labels"].numpy(), t["rel_triplets"].numpy()) for t in targets]
    got = whole([dense(t) for t in targets]).fg_matrix()
    assert got.sum() > 0 and np.array_equal(got, RI.count(split))
    assert np.array_equal(got, whole(targets).fg_matrix())
    # on an image WITH a duplicate the two forms differ by exactly the repeats
    dup = next(t for t in RI.train_targets() if len(torch.unique(t["rel_triplets"], dim=0)) < len(t["rel_triplets"]))
    assert whole([dup]).fg_matrix().sum() == len(dup["rel_triplets"])
    assert whole([dense(dup)]).fg_matrix().sum() == len(torch.unique(dup["rel_triplets"], dim=0))


def test_model_tables_from_the_counts(g):
    import helpers as Hh
    from egtr_amd.egtr import DetrForSceneGraphGeneration
    cfg_dict = dict(num_queries=12, encoder_layers=1, decoder_layers=1, dropout=0.0, auxiliary_loss=False,
                    num_labels=RI.C, num_rel_labels=RI.R, ce_loss_coefficient=2.0, rel_loss_coefficient=15.0,
                    connectivity_loss_coefficient=30.0, smoothing=1e-14, rel_sample_negatives=80,
                    rel_sample_nonmatching=80, rel_sample_negatives_largest=True, rel_sample_nonmatching_largest=True,
                    use_freq_bias=True, use_log_softmax=False, freq_bias_eps=1e-12, logit_adjustment=True,
                    logit_adj_tau=0.3)
    models = []
    for fg in (whole().fg_matrix(), g["fg_vg"]):
        torch.manual_seed(0)
        models.append(DetrForSceneGraphGeneration(Hh.product_config(cfg_dict), fg_matrix=fg))
    assert torch.equal(models[0].rel_dist, models[1].rel_dist) and float(models[0].rel_dist.sum()) > 0.99
    assert torch.equal(models[0].triplet_dist, models[1].triplet_dist)


def test_merge_of_two_halves(g):
    targets = RI.train_targets()
    a, b = whole(targets[:17]), whole(targets[17:])
    assert a.merge(b) is a
    assert np.array_equal(a.fg_matrix(), g["fg_vg"])
    with pytest.raises(ValueError):
        a.merge(RelationStatistics(RI.C + 1, RI.R))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_all_reduce_two_ranks_gloo(g, tmp_path):
    port = _free_port()
    outs = [str(tmp_path / f"rank{r}.npy") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_rel_stats_worker.py"), str(r), "2", str(port), outs[r]])
             for r in range(2)]
    for p in procs:
        assert p.wait(timeout=120) == 0
    for o in outs:
        assert np.array_equal(np.load(o), g["fg_vg"])


@pytest.mark.parametrize("bad", ["subject", "object", "negative", "predicate", "class"])
def test_out_of_range_raises_and_leaves_the_counts(g, bad):
    st = whole()
    before = st.counts.clone()
    t = {"class_labels": torch.tensor([0, 1, 2]), "rel_triplets": torch.tensor([[0, 1, 2], [1, 2, 0], [2, 0, 1]])}
    if bad == "subject":
        t["rel_triplets"][1, 0] = 3
    elif bad == "object":
        t["rel_triplets"][1, 1] = 3
    elif bad == "negative":
        t["rel_triplets"][1, 0] = -1
    elif bad == "predicate":
        t["rel_triplets"][1, 2] = RI.R
    else:
        t["class_labels"][1] = RI.C + 1
    good = RI.train_targets()[0]
    with pytest.raises(ValueError):
        st.update([good, t, good])
    assert torch.equal(st.counts, before)
    assert np.array_equal(st.fg_matrix(), g["fg_vg"])      # the host path raised at once: nothing is pending


def test_seen_bits_agree_with_the_counts(g):
    st = whole()
    bits = st.seen_bits()
    n = g["fg_vg"].size
    assert bits.dtype == torch.int64 and bits.shape == ((n + 63) // 64,)
    flat = g["fg_vg"].reshape(-1) > 0
    got = [bool((int(bits[i >> 6]) >> (i & 63)) & 1) for i in range(n)]
    assert got == flat.tolist()
    assert all(((int(bits[-1]) >> b) & 1) == 0 for b in range(n & 63, 64))       # the padding bits stay clear
    # bit 63 of a word is its sign bit
    assert seen_bits_host(torch.ones(64, dtype=torch.int64)).tolist() == [-1]
    assert seen_bits_host(torch.tensor([0] * 63 + [5])).tolist() == [-(1 << 63)]


def evaluator(mode, train_counts, **kw):
    return SceneGraphRecall(RI.R, multiple_preds=(mode == "m"), train_counts=train_counts, **kw)


def run(ev, cands, targets, bs=RI.N_TEST):
    for i in range(0, len(cands), bs):
        ev.update(cands[i:i + bs], targets[i:i + bs])
    return ev


@pytest.mark.parametrize("top,prefix", [(None, ""), (10, "k10_")])
@pytest.mark.parametrize("mode", ["m", "s"])
def test_host_zero_shot_matches_reference(g, split, mode, top, prefix):
    cands, targets, _ = split
    ev = run(evaluator(mode, whole(), keep_per_image=True), RI.candidates(cands, mode, top=top), targets)
    assert np.array_equal(ev.per_image_zero_shot().numpy(), g[f"{prefix}{mode}_zs_recall"])        # bit-equal rows
    got = ev.zero_shot()
    for j, k in enumerate(KS):
        assert abs(got[f"zR@{k}"] - g[f"{prefix}{mode}_zs_stats"][j]) <= 1e-12
    nz = g["n_zero_shot"]
    assert ev.n_zero_shot_images == int((nz > 0).sum()) and ev.n_zero_shot_triplets == int(nz.sum())
    if top is None:
        assert np.array_equal(ev.per_image().numpy(), g[f"{mode}_recall"])
        assert got["zR@20"] != ev.compute()["R@20"]


@pytest.mark.parametrize("mode", ["m", "s"])
def test_train_counts_forms_and_batch_sizes_agree(g, split, mode):
    cands, targets, _ = split
    c = RI.candidates(cands, mode)
    st = whole()
    base = run(evaluator(mode, st), c, targets)
    for tc, kw in ((g["fg_vg"], {}), (torch.from_numpy(g["fg_vg"]), {}), (st.seen_bits(), {"train_num_labels": RI.C})):
        for bs in (1, 5):
            ev = run(evaluator(mode, tc, **kw), c, targets, bs=bs)
            assert torch.equal(ev.zs_acc, base.zs_acc) and torch.equal(ev.acc, base.acc)
    a = run(evaluator(mode, st), c[:5], targets[:5])
    a.merge(run(evaluator(mode, st), c[5:], targets[5:]))
    assert torch.allclose(a.zs_acc, base.zs_acc, rtol=0, atol=1e-12) and a.n_zero_shot_triplets == base.n_zero_shot_triplets


@pytest.mark.parametrize("mode", ["m", "s"])
def test_without_train_counts_nothing_changes(split, mode):
    cands, targets, _ = split
    c = RI.candidates(cands, mode)
    today = run(SceneGraphRecall(RI.R, multiple_preds=(mode == "m"), keep_per_image=True), c, targets)
    none = run(evaluator(mode, None, keep_per_image=True), c, targets)
    with_counts = run(evaluator(mode, whole(), keep_per_image=True), c, targets)
    for ev in (none, with_counts):
        assert ev.width == today.width and torch.equal(ev.acc, today.acc)
        assert ev.compute() == today.compute() and ev.mean_recall() == today.mean_recall()
        assert torch.equal(ev.per_image(), today.per_image())
    assert none.zs_acc is None
    with pytest.raises(RuntimeError):
        none.zero_shot()


def test_no_zero_shot_triplet_gives_nan(g, split):
    cands, targets, _ = split
    idx = [i for i, n in enumerate(g["n_zero_shot"]) if n == 0]
    ev = evaluator("m", whole())
    assert all(math.isnan(v) for v in ev.zero_shot().values())
    ev.update([RI.candidates(cands, "m")[i] for i in idx], [targets[i] for i in idx])
    assert ev.n_images == len(idx) and not ev.zs_acc.any()
    assert all(math.isnan(v) for v in ev.zero_shot().values())


def test_bad_train_counts():
    with pytest.raises(ValueError):
        SceneGraphRecall(RI.R + 1, train_counts=whole())
    with pytest.raises(ValueError):
        SceneGraphRecall(RI.R, train_counts=np.zeros((3, 4, RI.R), np.int64))
    with pytest.raises(ValueError):
        SceneGraphRecall(RI.R, train_counts=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError):
        SceneGraphRecall(RI.R, train_counts=torch.zeros(2, dtype=torch.int64), train_num_labels=RI.C)
