"""CPU: the PredCls / SGCls candidate builder (runtime.matched_topk_host, runtime.matched_triplet_candidates) against the
reference's recorded evaluators (tests/golden/protocols_eval.npz, make_golden_protocols.py): candidate lists exact,
per-image recalls bit-equal; the defined order against a brute-force sort (tests/protocols_cases.py); padding; evaluate()
with the new flags; the C entry's argument checks."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import protocols_cases as PC  # noqa: E402
import protocols_eval_inputs as PI  # noqa: E402

from egtr_amd.evaluation import SceneGraphRecall, evaluate, first_ranks_host, gt_entry  # noqa: E402
from egtr_amd.runtime import matched_topk_host, matched_triplet_candidates  # noqa: E402

KS = (20, 50, 100)
PROTOCOLS = ("predcls", "sgcls")
MODES = (("m", "multiple"), ("s", "single"))
B = len(PI.GS)


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "protocols_eval.npz"))


@pytest.fixture(scope="module")
def inputs(g):
    return PI.protocols_eval_inputs(int(g["seed"]))


def candidates(inputs, protocol, mode, images=None):
    outputs, targets, query_of = inputs
    images = list(range(B)) if images is None else images
    outs = {k: v[images] for k, v in outputs.items()}
    return matched_triplet_candidates(outs, [targets[i] for i in images], PI.FixedMatcher([query_of[i] for i in images]),
                                      PI.NUM_LABELS, 100, mode=mode, protocol=protocol), [targets[i] for i in images]


@pytest.mark.parametrize("protocol", PROTOCOLS)
@pytest.mark.parametrize("m,mode", MODES)
def test_host_twin_reproduces_the_reference_lists(g, inputs, protocol, m, mode):
    outputs, targets, query_of = inputs
    for j in range(B):
        G = PI.GS[j]
        qof = torch.full((1, G + 1), -1, dtype=torch.int32)
        qof[0, :G] = torch.from_numpy(query_of[j])
        obj = torch.zeros(1, G + 1)
        obj[0, :G] = torch.from_numpy(g[f"{protocol}_{m}{j}_obj_scores"])
        inds, rs, ts, count = matched_topk_host(outputs["pred_rel"][j:j + 1], outputs["pred_connectivity"][j:j + 1], qof,
                                                obj, 100, 0 if m == "m" else 1)
        want = g[f"{protocol}_{m}{j}_pred_rel_inds"]
        n = want.shape[0]
        assert int(count[0]) == n == min(100, G * (G - 1) * (PI.R if m == "m" else 1))
        assert np.array_equal(inds[0, :n].numpy(), want)
        assert np.array_equal(rs[0, :n].numpy(), g[f"{protocol}_{m}{j}_rel_scores"])
        assert np.array_equal(ts[0, :n].numpy(), g[f"{protocol}_{m}{j}_triplet_scores"])
        assert (inds[0, n:] == G).all() and (rs[0, n:] == 0).all() and (ts[0, n:] == 0).all()
    assert min(g[f"{protocol}_{m}{j}_pred_rel_inds"].shape[0] for j in range(B)) == (12 if m == "m" else 2)


@pytest.mark.parametrize("protocol", PROTOCOLS)
@pytest.mark.parametrize("m,mode", MODES)
def test_candidates_reproduce_the_reference_recalls(g, inputs, protocol, m, mode):
    cands, targets = candidates(inputs, protocol, mode)
    for j, (c, t) in enumerate(zip(cands, targets)):
        e, G = gt_entry(t), PI.GS[j]
        assert c["pred_boxes"].shape == (17, 4) and c["pred_rel_inds"].shape[0] == 100
        assert torch.equal(c["pred_boxes"][:G], e["gt_boxes"]) and (c["pred_boxes"][G:] == 0).all()
        assert np.array_equal(c["pred_classes"][:G].numpy(), g[f"{protocol}_{m}{j}_pred_classes"])
        assert (c["pred_classes"][G:] == -1).all()
        assert np.array_equal(c["obj_scores"][:G].numpy(), g[f"{protocol}_{m}{j}_obj_scores"])
    ev = SceneGraphRecall(PI.R, ks=KS, multiple_preds=(m == "m"), keep_per_image=True)
    ev.update(cands, targets)
    assert np.array_equal(ev.per_image().numpy(), g[f"{protocol}_{m}_recall"])       # bit-equal per-image recalls
    got = dict(ev.compute(), **ev.mean_recall())
    for i, k in enumerate(KS):
        assert abs(got[f"R@{k}"] - g[f"{protocol}_{m}_stats"][i]) <= 1e-12
        assert abs(got[f"mR@{k}"] - g[f"{protocol}_{m}_mr"][i]) <= 1e-12
    nk, want_pp = len(KS), g[f"{protocol}_{m}_pred_recall"]        # per-image per-predicate recalls, bit for bit
    for j, (c, t) in enumerate(zip(cands, targets)):
        e = SceneGraphRecall(PI.R, ks=KS, multiple_preds=(m == "m"))
        e.update([c], [t])
        for p in range(PI.R):
            if e.acc[e._fbase + p] == 0:
                assert np.isnan(want_pp[p, j]).all()
            else:
                assert np.array_equal(e.acc[e._pbase + p * nk:e._pbase + (p + 1) * nk].numpy(), want_pp[p, j])


def test_fixture_is_nontrivial(g, inputs):
    _, targets, _ = inputs
    for protocol in PROTOCOLS:
        rec = g[f"{protocol}_m_recall"]
        assert (rec[:, 0] < rec[:, 2]).sum() >= 3 and (rec[:, 0] < rec[:, 1]).any() and (rec[:, 1] < rec[:, 2]).any()
        assert np.isnan(g[f"{protocol}_m_pred_stats"][-1]).all()                # a predicate that never occurs
    assert (g["sgcls_m_recall"] <= g["predcls_m_recall"]).all()                 # wrong classes only lose triplets
    assert (g["sgcls_m_recall"] < g["predcls_m_recall"]).any()
    wrong = sum(int((g[f"sgcls_m{j}_pred_classes"] != g[f"{j}_gt_classes"]).sum()) for j in range(B))
    assert wrong >= 5
    for j in PI.DUP:       # the candidate on GT object 1 matches the GT triplet on its near-copy, object 0
        e = gt_entry(targets[j])
        rels = e["gt_relations"]
        t = [i for i, r in enumerate(rels.tolist()) if r[:2] == [0, 2]]
        assert len(t) == 1 and [1, 2] not in [r[:2] for r in rels.tolist()]
        lst = torch.from_numpy(g[f"predcls_m{j}_pred_rel_inds"])
        fr = first_ranks_host(lst, e["gt_boxes"], e["gt_classes"], rels, e["gt_boxes"], e["gt_classes"])
        hit = int(fr[t[0]])
        assert hit < 20 and lst[hit].tolist() == [1, 2, int(rels[t[0], 2])]


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_zero_shot_rows_equal_those_of_the_unpadded_lists(g, inputs, protocol):
    _, targets, _ = inputs
    rng = np.random.Generator(np.random.PCG64(3))
    fg = torch.from_numpy((rng.random((PI.NUM_LABELS + 1, PI.NUM_LABELS + 1, PI.R)) < 0.5).astype(np.int64))
    for m, mode in MODES:
        cands, _ = candidates(inputs, protocol, mode)
        ev = SceneGraphRecall(PI.R, ks=KS, multiple_preds=(m == "m"), keep_per_image=True, train_counts=fg)
        ev.update(cands, targets)
        ref = SceneGraphRecall(PI.R, ks=KS, multiple_preds=(m == "m"), keep_per_image=True, train_counts=fg)
        for j, t in enumerate(targets):        # the reference's unpadded lists, GT boxes as pred_boxes
            e = gt_entry(t)
            ref.update([{"pred_boxes": e["gt_boxes"],
                         "pred_classes": torch.from_numpy(g[f"{protocol}_{m}{j}_pred_classes"]),
                         "pred_rel_inds": torch.from_numpy(g[f"{protocol}_{m}{j}_pred_rel_inds"]),
                         "rel_scores": torch.from_numpy(g[f"{protocol}_{m}{j}_rel_scores"])}], [t])
        assert ref.n_zero_shot_triplets > 5 and torch.equal(ev.zs_acc, ref.zs_acc)
        assert torch.equal(ev.per_image_zero_shot(), ref.per_image_zero_shot())
        assert torch.equal(ev.per_image(), ref.per_image())


@pytest.mark.parametrize("protocol", PROTOCOLS)
@pytest.mark.parametrize("m,mode", MODES)
def test_padding_is_neutral(inputs, protocol, m, mode):
    cands, targets = candidates(inputs, protocol, mode)
    whole = SceneGraphRecall(PI.R, ks=KS, multiple_preds=(m == "m"), keep_per_image=True)
    whole.update(cands, targets)
    alone = SceneGraphRecall(PI.R, ks=KS, multiple_preds=(m == "m"), keep_per_image=True)
    for j in range(B):
        c1, t1 = candidates(inputs, protocol, mode, images=[j])
        assert c1[0]["pred_boxes"].shape[0] == PI.GS[j] + 1
        n = min(100, PI.GS[j] * (PI.GS[j] - 1) * (PI.R if m == "m" else 1))
        assert torch.equal(c1[0]["pred_rel_inds"][:n], cands[j]["pred_rel_inds"][:n])     # the order does not depend on Gp
        assert (c1[0]["pred_rel_inds"][n:] == PI.GS[j]).all() and (cands[j]["pred_rel_inds"][n:] == 16).all()
        alone.update(c1, t1)
    assert torch.equal(torch.cat(whole._per_image), torch.cat(alone._per_image))
    assert torch.equal(whole.acc, alone.acc)


@pytest.mark.parametrize("name", sorted(PC.definition_cases()))
@pytest.mark.parametrize("mode", [0, 1])
def test_host_twin_follows_the_definition(name, mode):
    rel, conn, qof, obj, K = PC.definition_cases()[name]
    got = matched_topk_host(rel, conn, qof, obj, K, mode)
    want = PC.brute_force(rel, conn, qof, obj, K, mode)
    assert PC.same(got, want)
    count = want[3]
    if name == "M_0_and_1":
        assert count.tolist() == [0, 0] and (got[0] == qof.shape[1] - 1).all()
    if name == "K_above_domain":
        assert (count < K).all() and (count > 0).all()
    if name == "all_scores_zero":        # every score ties: the list is the domain in ascending (s, o, p)
        rows = got[0][0].tolist()
        assert rows == sorted(rows) and (got[2] == 0).all()
    if name == "nan_and_negative_zero":
        ts = want[2][0, :int(count[0])]
        assert ts.isnan().any() and not ts[:int((~ts.isnan()).sum())].isnan().any()      # NaN scores come last


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def test_evaluate_flags(g, inputs):
    outputs, targets, query_of = inputs
    batches = [{"pixel_values": torch.zeros(B, 3, 8, 8), "pixel_mask": torch.ones(B, 8, 8), "labels": targets}]
    args = (_Stub(), batches, PI.NUM_LABELS, PI.R)
    kw = dict(graphed=False, forward=lambda pv, pm: outputs, matcher=PI.FixedMatcher(query_of))
    base = evaluate(*args, single=True, multiple=True, **kw)
    assert evaluate(*args, single=True, multiple=True, predcls=False, sgcls=False, **kw) == base
    more = evaluate(*args, single=True, multiple=True, predcls=True, sgcls=True, **kw)
    assert {k: v for k, v in more.items() if k in base} == base
    new = {f"{pre}{proto}_{met}@{k}" for pre in ("", "(single)") for proto in PROTOCOLS for met in ("R", "mR")
           for k in KS}
    assert set(more) - set(base) == new
    for proto in PROTOCOLS:
        for i, k in enumerate(KS):
            assert abs(more[f"{proto}_R@{k}"] - g[f"{proto}_m_stats"][i]) <= 1e-12
            assert abs(more[f"(single){proto}_mR@{k}"] - g[f"{proto}_s_mr"][i]) <= 1e-12
    only = evaluate(*args, single=False, multiple=True, predcls=True, **kw)
    assert set(only) == {f"{met}@{k}" for met in ("R", "mR") for k in KS} | {
        f"predcls_{met}@{k}" for met in ("R", "mR") for k in KS}
    fg = torch.ones(PI.NUM_LABELS + 1, PI.NUM_LABELS + 1, PI.R, dtype=torch.int64)
    zs = evaluate(*args, single=False, multiple=True, sgcls=True, train_counts=fg, **kw)
    assert {f"sgcls_zR@{k}" for k in KS} <= set(zs)
    with pytest.raises(ValueError):
        evaluate(*args, single=False, multiple=False, phrdet=True, predcls=True, **kw)
    with pytest.raises(ValueError):
        evaluate(*args, single=False, multiple=False, sgcls=True, **kw)
    with pytest.raises(ValueError):
        matched_triplet_candidates(outputs, targets, kw["matcher"], PI.NUM_LABELS, mode="oi")
    with pytest.raises(ValueError):
        matched_triplet_candidates(outputs, targets, kw["matcher"], PI.NUM_LABELS, protocol="sgdet")


def test_c_entry_rejects_bad_arguments_without_a_gpu():
    from egtr_amd import _lib
    h = _lib.lib()
    P = ctypes.c_void_p
    ok = [P(64)] * 4                                   # never dereferenced: the checks come before any HIP call
    out = [P(64)] * 5

    def call(ptrs, B=1, N=16, R=6, Gp=8, K=20, mode=0, outs=out):
        return h.egtr_matched_topk_f32(None, *ptrs, B, N, R, Gp, K, mode, *outs)

    assert call([None, None, None, None], outs=[None] * 5) == -1
    assert call([P(64), None, None, P(64)]) == -1              # query_of missing
    assert call(ok, outs=[None] + out[1:]) == -1               # no workspace
    assert call(ok, outs=out[:4] + [None]) == -1               # no count
    assert call(ok, K=0) == -1 and call(ok, K=1025) == -1 and call(ok, R=257) == -1
    assert call(ok, mode=2) == -1 and call(ok, B=-1) == -1 and call(ok, N=0) == -1 and call(ok, Gp=0) == -1
    assert call(ok, B=0) == 0                                  # an empty batch is no error and no launch
    assert h.egtr_matched_topk_workspace_bytes(1, 8, 1025) == -1
    assert h.egtr_matched_topk_workspace_bytes(2, 201, 100) >= 2 * 100 * 8
    assert h.egtr_abi_version() == 7
