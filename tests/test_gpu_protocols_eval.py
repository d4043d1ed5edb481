"""GPU: the matched top-K kernel (csrc/matched_topk.hip, ``ops.matched_topk``) against its torch twin
(``runtime.matched_topk_host``) -- indices, both score outputs and the counts exact -- and the device path of
``runtime.matched_triplet_candidates`` into the device ``SceneGraphRecall``: per-image recalls bit-equal to the
reference's recorded PredCls / SGCls evaluators (tests/golden/protocols_eval.npz), accumulators and first ranks equal to
the host path's; the mapping through the real device matcher; ``evaluate`` with the new flags."""
import math
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

from egtr_amd import ops  # noqa: E402
from egtr_amd.deformable_detr import DeformableDetrHungarianMatcher  # noqa: E402
from egtr_amd.evaluation import SceneGraphRecall, evaluate, first_ranks_host, gt_entry, numpy_argmax  # noqa: E402
from egtr_amd.runtime import _matched_query_of, matched_topk_host, matched_triplet_candidates  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KS = (20, 50, 100)
PROTOCOLS = ("predcls", "sgcls")
MODES = (("m", "multiple"), ("s", "single"))


def dev(x):
    return None if x is None else x.to(DEV)


def kernel(rel, conn, qof, obj, K, mode):
    return ops.matched_topk(dev(rel), dev(conn), dev(qof), dev(obj), K, mode)


# (B, N, R, matched per image, K).  The kernel cuts the Gp^2 pairs of an image into min(256, ceil(Gp^2 / 128)) slices: one
# slice; a batch with empty, one-object and full images (3 slices); 14 slices with K at its limit (every survivor of every
# slice reaches the merge); the production shape
SHAPES = [(1, 16, 6, (7,), 20), (4, 16, 6, (0, 1, 12, 16), 100), (2, 40, 50, (40, 40), 1024), (1, 200, 50, (30,), 100)]


@pytest.mark.parametrize("conn", [True, False])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B,N,R,matched,K", SHAPES)
def test_kernel_equals_torch_twin(B, N, R, matched, K, mode, conn):
    Gp = max(matched) + 1
    rel, cn, qof, obj = PC.random_inputs(11 + N + mode, B, N, R, Gp, matched, conn=conn)
    got = kernel(rel, cn, qof, obj, K, mode)
    want = matched_topk_host(rel, cn, qof, obj, K, mode)
    assert PC.same(got, want)
    entries = [m * (m - 1) * (R if mode == 0 else 1) for m in matched]
    assert got[3].tolist() == [min(K, e) for e in entries]
    if mode == 0 and R == 50:      # the clamp makes r = 1 for several of a pair's 50 predicates: ties inside the list
        ts = want[2][0, :int(want[3][0])]
        assert (ts[1:] == ts[:-1]).any()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", sorted(PC.definition_cases()))
def test_kernel_follows_the_definition(name, mode):
    rel, conn, qof, obj, K = PC.definition_cases()[name]
    assert PC.same(kernel(rel, conn, qof, obj, K, mode), PC.brute_force(rel, conn, qof, obj, K, mode))


def test_equal_scores_across_a_digit_boundary_of_the_select():
    """All scores are 0, so the whole domain ties and the list is the domain in ascending flat index; K is chosen so that
    rank K - 1 is flat index 1023 and rank K is 1024: the two order words differ first at bit 10, the boundary between
    the last two digits of the radix select."""
    N, R, Gp = 16, 6, 17
    rel, _, qof, obj = PC.random_inputs(5, 1, N, R, Gp, (16,), conn=False)
    qof[0, :16], qof[0, 16] = torch.arange(16, dtype=torch.int32), -1
    flats = [(s * Gp + o) * R + p for s in range(16) for o in range(16) if s != o for p in range(R)]
    K = sum(f <= 1023 for f in flats)
    assert flats[K - 1] == 1023 and flats[K] == 1024 and K <= 1024
    rel = torch.full_like(rel, -1.0)
    got = kernel(rel, None, qof, obj, K, 0)
    assert PC.same(got, matched_topk_host(rel, None, qof, obj, K, 0))
    s, o, p = got[0][0, -1].tolist()
    assert (s * Gp + o) * R + p == 1023 and int(got[3][0]) == K


def test_adjacent_scores_across_a_bucket_boundary_of_the_select():
    """Ranks K - 1 and K hold 0.5 and the float just below it: their keys 0xBF000000 and 0xBEFFFFFF differ in every digit
    of the select."""
    N, R, Gp, K = 16, 6, 17, 40
    rel, _, qof, obj = PC.random_inputs(6, 1, N, R, Gp, (16,), conn=False)
    rng = np.random.Generator(np.random.PCG64(8))
    vals = np.full(N * N * R, 0.25, np.float32)
    qs, qo = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    off = np.repeat((qs != qo).ravel(), R).nonzero()[0]               # every query is matched: all off-diagonal cells
    pick = rng.choice(off, 2 * K, replace=False)
    vals[pick[:K]] = 0.5
    vals[pick[K:]] = np.nextafter(np.float32(0.5), np.float32(0))
    rel = torch.from_numpy(vals).reshape(1, N, N, R)
    obj = torch.ones_like(obj)
    got = kernel(rel, None, qof, obj, K, 0)
    assert PC.same(got, matched_topk_host(rel, None, qof, obj, K, 0))
    assert (got[2].cpu() == 0.5).all()
    more = kernel(rel, None, qof, obj, K + 1, 0)
    assert float(more[2][0, K]) == float(np.nextafter(np.float32(0.5), np.float32(0)))


# ---- the fixture through the device path -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "protocols_eval.npz"))


@pytest.fixture(scope="module")
def inputs(g):
    return PI.protocols_eval_inputs(int(g["seed"]))


@pytest.mark.parametrize("protocol", PROTOCOLS)
@pytest.mark.parametrize("m,mode", MODES)
def test_device_path_reproduces_the_reference_recalls(g, inputs, protocol, m, mode):
    outputs, targets, query_of = inputs
    matcher = PI.FixedMatcher(query_of)
    on_dev = {k: v.to(DEV) for k, v in outputs.items()}
    cands = matched_triplet_candidates(on_dev, targets, matcher, PI.NUM_LABELS, 100, mode=mode, protocol=protocol)
    host_cands = matched_triplet_candidates(outputs, targets, matcher, PI.NUM_LABELS, 100, mode=mode, protocol=protocol)
    for c, h in zip(cands, host_cands):
        assert c["pred_rel_inds"].is_cuda and torch.equal(c["pred_rel_inds"].cpu(), h["pred_rel_inds"])
        assert torch.equal(c["pred_boxes"].cpu(), h["pred_boxes"])
        assert torch.equal(c["pred_classes"].cpu(), h["pred_classes"])
    multiple = m == "m"
    ev = SceneGraphRecall(PI.R, ks=KS, multiple_preds=multiple, keep_per_image=True)
    ev.update(cands, targets)
    host = SceneGraphRecall(PI.R, ks=KS, multiple_preds=multiple, keep_per_image=True)
    host.update(host_cands, targets)
    assert np.array_equal(ev.per_image().numpy(), g[f"{protocol}_{m}_recall"])        # the reference's, bit for bit
    assert torch.equal(ev.acc.cpu(), host.acc)
    want = []
    for c, t in zip(host_cands, targets):
        e = gt_entry(t)
        rels = c["pred_rel_inds"] if multiple else torch.cat(
            [c["pred_rel_inds"], numpy_argmax(c["rel_scores"])[:, None]], 1)
        want.append(first_ranks_host(rels, c["pred_boxes"], c["pred_classes"], e["gt_relations"], e["gt_boxes"],
                                     e["gt_classes"]))
    assert torch.equal(ev.last_first_rank.cpu().long(), torch.cat(want))


def _random_outputs(seed, B, N, R, C):
    gen = torch.Generator().manual_seed(seed)
    return {"logits": torch.randn(B, N, C + 1, generator=gen), "pred_boxes": torch.rand(B, N, 4, generator=gen) * 0.4 + 0.3,
            "pred_rel": torch.rand(B, N, N, R, generator=gen) * 1.4 - 0.2,
            "pred_connectivity": torch.rand(B, N, N, 1, generator=gen) * 1.4 - 0.2}


def _random_targets(seed, Gs, R, C):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for G in Gs:
        rel = (torch.rand(G, G, R, generator=gen) < 0.15).float()
        rel[torch.arange(G), torch.arange(G)] = 0
        rel[0, 1, 0] = 1
        out.append(dict(class_labels=torch.randint(0, C, (G,), generator=gen),
                        boxes=torch.rand(G, 4, generator=gen) * 0.4 + 0.3, rel=rel, orig_size=torch.tensor([64, 64])))
    return out


def test_mapping_through_the_device_matcher():
    B, N, R, C = 3, 16, 4, 5
    outputs = {k: v.to(DEV) for k, v in _random_outputs(5, B, N, R, C).items()}
    targets = _random_targets(6, (3, 9, 5), R, C)
    matcher = DeformableDetrHungarianMatcher(class_cost=2.0, bbox_cost=5.0, giou_cost=2.0)
    Gp = 10
    qof = _matched_query_of(outputs, targets, matcher, C, Gp).cpu()
    matched = matcher({"logits": outputs["logits"][..., :C], "pred_boxes": outputs["pred_boxes"]}, targets)[0]
    for b, (pred_idx, tgt_idx) in enumerate(matched):
        want = torch.full((Gp,), -1, dtype=torch.int32)
        for q, t in zip(pred_idx.tolist(), tgt_idx.tolist()):
            want[t] = q
        assert torch.equal(qof[b], want) and int((want >= 0).sum()) == len(targets[b]["class_labels"])
    cands = matched_triplet_candidates(outputs, targets, matcher, C, 30, mode="multiple", protocol="sgcls")
    rel = outputs["pred_rel"].clamp(0, 1) * outputs["pred_connectivity"].clamp(0, 1)
    scores, classes = torch.max(outputs["logits"].softmax(-1)[..., :C], -1)
    for b, c in enumerate(cands):
        G, q = len(targets[b]["class_labels"]), qof[b].long().to(DEV)
        assert torch.equal(c["pred_classes"][:G], classes[b][q[:G]]) and (c["pred_classes"][G:] == -1).all()
        assert torch.equal(c["obj_scores"][:G], scores[b][q[:G]])
        s, o, p = c["pred_rel_inds"].unbind(-1)
        n = min(30, G * (G - 1) * R)
        assert torch.equal(c["rel_scores"][:n], rel[b, q[s[:n]], q[o[:n]], p[:n]])
        assert (c["pred_rel_inds"][n:] == Gp - 1).all()


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def test_evaluate_on_device_equals_the_host_copy():
    """Two batches with different G.  The device call runs the real device matcher; the host call gets its assignment
    (a FixedMatcher), so that the comparison is about candidates and evaluators, not about two Hungarian solvers."""
    N, R, C = 16, 4, 5
    outs = [_random_outputs(21, 2, N, R, C), _random_outputs(22, 3, N, R, C)]
    tgts = [_random_targets(23, (4, 7), R, C), _random_targets(24, (12, 2, 6), R, C)]
    matcher = DeformableDetrHungarianMatcher(class_cost=2.0, bbox_cost=5.0, giou_cost=2.0)
    fg = torch.zeros(C + 1, C + 1, R, dtype=torch.int64)
    fg[::2] = 1
    fixed = []                                             # the device matcher's assignment, per batch and image
    for o, t in zip(outs, tgts):
        od = {k: v.to(DEV) for k, v in o.items()}
        pairs = matcher({"logits": od["logits"][..., :C], "pred_boxes": od["pred_boxes"]}, t)[0]
        fixed.append([dict(zip(ti.tolist(), pi.tolist())) for pi, ti in pairs])
    calls = {"i": 0}

    def host_matcher(outputs, targets):
        maps = fixed[calls["i"] // 4]                      # four candidate lists per batch: 2 protocols x 2 modes
        calls["i"] += 1
        return PI.FixedMatcher([np.array([mp[g] for g in range(len(mp))]) for mp in maps])(outputs, targets)

    results = []
    for device, m in ((DEV, matcher), (torch.device("cpu"), host_matcher)):
        state = {"i": 0}

        def forward(pv, pm):
            o = {k: v.to(device) for k, v in outs[state["i"]].items()}
            state["i"] += 1
            return o

        batches = [{"pixel_values": torch.zeros(len(t), 3, 8, 8), "pixel_mask": torch.ones(len(t), 8, 8), "labels": t}
                   for t in tgts]
        results.append(evaluate(_Stub().to(device), batches, C, R, single=True, multiple=True, graphed=False,
                                forward=forward, matcher=m, predcls=True, sgcls=True, train_counts=fg))
    got, want = results
    new = [k for k in got if "predcls_" in k or "sgcls_" in k]
    assert len(new) == 2 * 2 * 3 * len(KS) and set(got) == set(want)
    for k in new:
        assert got[k] == want[k] or (math.isnan(got[k]) and math.isnan(want[k])), k
    assert 0 < got["predcls_R@100"] <= 1
