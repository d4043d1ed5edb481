"""GPU (-m gpu): relation targets as triplets / bit-packed words -- the pack kernel against the CPU
composition, egtr_relation_loss_f32 on the words bit-identical to itself on the dense form of the same targets
and within the oracle's tolerance, one training step and one evaluation of the small model with both target forms."""
import functools
import json

import pytest
import torch

import helpers as Hh
import weights as W
from oracle import loss as OL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_SAMPLE = 80

# (N, R, per-image (targets, triplets drawn)): image 0 carries duplicated triplets, image 1 no relation, image 2 no target at
# all (T = 0).  The fourth image of the last case exists for the bounds of the selection count, see test_selection_bounds.
CASES = {
    "n7r5": (7, 5, ((4, 6), (3, 0), (0, 0))),
    "n70r50": (70, 50, ((9, 14), (20, 0), (0, 0))),
    "n33r64": (33, 64, ((8, 12), (5, 0), (0, 0))),
    "n70r50-bounds": (70, 50, ((3, 9), (20, 0), (0, 0), (30, 12))),
}
BASE = ("n7r5", "n70r50", "n33r64")


def dense_reference_way(triplets, N, R):
    """data/visual_genome.py:74-80: zeros, then one indexed assignment."""
    rel = torch.zeros([N, N, R])
    idx = triplets.T
    rel[idx[0, :], idx[1, :], idx[2, :]] = 1.0
    return rel


def distinct_logits(g, *shape):
    """Random fp32 logits in (-4, 4) without two equal values: a random permutation of an evenly spaced grid (independent
    normal draws collide at these sizes).  Tickets among EQUAL keys are the one place where two correct runs may differ."""
    n = 1
    for s in shape:
        n *= s
    assert n < 2 ** 24
    x = ((torch.randperm(n, generator=g).float() + 0.5) / n - 0.5) * 8.0
    return x.view(*shape)


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs of one case (host), built once and left unchanged."""
    N, R, images = CASES[name]
    g = torch.Generator().manual_seed(1000 + N + R + len(images))
    B = len(images)
    trips, indices, costs = [], [], []
    for T, K in images:
        if K:
            so = torch.stack([torch.randint(0, T, (K,), generator=g), torch.randint(0, T, (K,), generator=g)], 1)
            t = torch.cat([so, torch.randint(0, R, (K, 1), generator=g)], 1)
            t[1] = t[0]                              # a duplicated triplet
            t[2, :2], t[2, 2] = t[0, :2], (t[0, 2] + 1) % R   # two predicates on one pair
            t[3, 2] = R - 1                          # the top bit of the word (bit 63 at R = 64)
        else:
            t = torch.zeros(0, 3, dtype=torch.int64)
        trips.append(t)
        indices.append((torch.randperm(N, generator=g)[:T].sort()[0], torch.randperm(T, generator=g)))
        costs.append(torch.randn(T, generator=g) * 3)
    pred_rel = distinct_logits(g, B, N, N, R)
    for b in range(B):
        assert pred_rel[b].unique().numel() == N * N * R      # no two logits of an image are equal
    pred_conn = torch.randn(B, N, N, 1, generator=g)
    dense = [dense_reference_way(t, N, R) for t in trips]
    return dict(N=N, R=R, B=B, trips=trips, dense=dense, indices=indices, costs=costs, pred_rel=pred_rel,
                pred_conn=pred_conn)


def matcher_flat(indices, costs):
    offs = [0]
    for a, _ in indices:
        offs.append(offs[-1] + int(a.shape[0]))
    pi = torch.cat([a for a, _ in indices]).to(DEV)
    ti = torch.cat([b for _, b in indices]).to(DEV)
    mc = torch.cat(list(costs)).float().to(DEV)
    if pi.numel() == 0:
        pi, ti, mc = (torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV),
                      torch.zeros(1, device=DEV))
    return pi, ti, mc, torch.tensor(offs, dtype=torch.int32).to(DEV)


def run_entries(c, indices=None):
    """(dense entry, packed entry) -> (loss [2], grad_rel, grad_conn) each, same matcher outputs."""
    from egtr_amd import ops, targets as T
    pr, pc = c["pred_rel"].to(DEV), c["pred_conn"].to(DEV)
    pi, ti, mc, off = matcher_flat(indices if indices is not None else c["indices"], c["costs"])
    nm = float(OL.nonmatching_cost(2.0, 5.0, 2.0, 1e-14))
    rels = [d.to(DEV) for d in c["dense"]]
    ptrs = torch.tensor([r.data_ptr() for r in rels], dtype=torch.int64).to(DEV)
    bits = T.pack_relations([{"rel_triplets": t} for t in c["trips"]], c["N"], c["R"], DEV)
    d = ops.relation_loss_launch(pr, pc, ptrs, False, pi, ti, mc, off, nm, K_SAMPLE, K_SAMPLE)
    p = ops.relation_loss_launch(pr, pc, bits, True, pi, ti, mc, off, nm, K_SAMPLE, K_SAMPLE)
    torch.cuda.synchronize()
    return [x.cpu() for x in d], [x.cpu() for x in p]


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------- pack kernel
@pytest.mark.parametrize("name", BASE)
def test_pack_kernel_equals_cpu_composition(name):
    from egtr_amd import targets as T
    c = case(name)
    N, R = c["N"], c["R"]
    want = T.pack_relations([{"rel_triplets": t} for t in c["trips"]], N, R, "cpu")
    for b in range(c["B"]):
        assert torch.equal(T.unpack_relations(want, b, R), c["dense"][b])
    host = T.pack_relations([{"rel_triplets": t} for t in c["trips"]], N, R, DEV)           # one pinned copy
    dev = T.pack_relations([{"rel_triplets": t.to(DEV)} for t in c["trips"]], N, R, DEV)    # triplets already on the device
    assert host.dtype == torch.int64 and tuple(host.shape) == (c["B"], N, N)
    assert torch.equal(host.cpu(), want) and torch.equal(dev.cpu(), want)
    s, o, _ = c["trips"][0][3].tolist()
    assert (int(want[0, s, o]) >> (R - 1)) & 1 == 1
    if R == 64:
        assert int(host[0, s, o]) < 0               # bit 63


@pytest.mark.parametrize("name", BASE)
def test_pack_kernel_drops_out_of_range_device_triplets(name):
    from egtr_amd import targets as T
    c = case(name)
    N, R = c["N"], c["R"]
    good = c["trips"][0]
    bad = torch.tensor([[N, 0, 0], [0, N, 0], [0, 0, R], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [N - 1, N - 1, 64],
                        [2 ** 40, 1, 1]])
    mixed = torch.cat([good[:2], bad[:4], good[2:], bad[4:]])
    tg = [{"rel_triplets": mixed.to(DEV)}, {"rel_triplets": bad.to(DEV)}, {"rel_triplets": good.to(DEV)}]
    got = T.pack_relations(tg, N, R, DEV).cpu()
    want = T.pack_relations([{"rel_triplets": good}, {"rel_triplets": good[:0]}, {"rel_triplets": good}], N, R, "cpu")
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------- loss entries
@pytest.mark.parametrize("name", list(CASES))
def test_packed_loss_entry_is_bit_identical_to_dense_entry(name):
    d, p = run_entries(case(name))
    assert torch.isfinite(d[0]).all()
    for a, b, what in zip(d, p, ("loss_out", "grad_rel", "grad_conn")):
        assert same_bits(a, b), what
    assert int((d[1] != 0).sum()) > 0


def test_selection_bounds():
    """80 n_true against the number of false candidates of the matched block (egtr:852-858): image 0 is capped by its
    candidates, image 3 is not; the gradient's support has exactly the predicted number of elements."""
    c = case("n70r50-bounds")
    N, R = c["N"], c["R"]
    n_sel = 0
    capped = []
    for (a, b), rel in zip(c["indices"], c["dense"]):
        T = int(a.shape[0])
        block = rel[b][:, b]
        n_true, n_false = int((block != 0).sum()), int((block != 1).sum())
        capped.append(n_true > 0 and K_SAMPLE * n_true > n_false)
        if n_true:
            n_sel += n_true + min(K_SAMPLE * n_true, n_false) + min(K_SAMPLE * n_true, (N * N - T * T) * R)
    assert capped == [True, False, False, False]
    b3 = c["dense"][3][c["indices"][3][1]][:, c["indices"][3][1]]
    assert 0 < K_SAMPLE * int((b3 != 0).sum()) < int((b3 != 1).sum())
    _, p = run_entries(c)
    # a true relation that is also among the sampled... cannot be: true relations are no false candidates; every selected
    # element has a non-zero gradient (sigmoid(x) - y = 0 needs y = sigmoid(x) exactly)
    assert int((p[1] != 0).sum()) == n_sel


@pytest.mark.parametrize("name", BASE)
def test_packed_route_vs_oracle(name):
    """ops.relation_losses on ``rel_triplets`` targets against oracle.loss.relation_losses in float64 under autograd:
    value 1e-5 relative, gradient 1e-7 absolute (the bounds of test_relation_loss_kernel_vs_oracle)."""
    from egtr_amd import ops
    c = case(name)
    nm_cost = OL.nonmatching_cost(2.0, 5.0, 2.0, 1e-14)
    pr64 = c["pred_rel"].double().requires_grad_(True)
    pc64 = c["pred_conn"].double().requires_grad_(True)
    w_rel, w_conn = OL.relation_losses(pr64, pc64, [{"rel": d.double()} for d in c["dense"]], c["indices"],
                                       [x.double() for x in c["costs"]], nm_cost, K_SAMPLE, K_SAMPLE, True)
    assert not bool(torch.isnan(w_rel))
    (w_rel * 1.5 + w_conn * 0.5).backward()
    prd = c["pred_rel"].to(DEV).requires_grad_(True)
    pcd = c["pred_conn"].to(DEV).requires_grad_(True)
    l_rel, l_conn = ops.relation_losses(prd, pcd, [{"rel_triplets": t} for t in c["trips"]],
                                        [(a.to(DEV), b.to(DEV)) for a, b in c["indices"]],
                                        [x.to(DEV) for x in c["costs"]], float(nm_cost), K_SAMPLE, K_SAMPLE)
    assert abs(float(l_conn) - float(w_conn)) < 1e-5 * max(1.0, abs(float(w_conn)))
    assert abs(float(l_rel) - float(w_rel)) < 1e-5 * max(1.0, abs(float(w_rel)))
    (l_rel * 1.5 + l_conn * 0.5).backward()
    assert (prd.grad.cpu().double() - pr64.grad).abs().max() < 1e-7
    assert (pcd.grad.cpu().double() - pc64.grad).abs().max() < 1e-7


@pytest.mark.parametrize("name", ["n7r5", "n70r50-bounds"])
def test_invalid_matcher_output_is_an_image_without_matches(name):
    """-1 indices (a cost matrix the matcher refused) for image 0: the packed entry does what the dense entry does, and
    both give what the same batch gives when that image has no matches at all."""
    c = case(name)
    a0, b0 = c["indices"][0]
    minus = [(torch.full_like(a0, -1), torch.full_like(b0, -1))] + list(c["indices"][1:])
    d, p = run_entries(c, minus)
    for a, b, what in zip(d, p, ("loss_out", "grad_rel", "grad_conn")):
        assert same_bits(a, b), what
    none = dict(c, indices=[(a0[:0], b0[:0])] + list(c["indices"][1:]), costs=[c["costs"][0][:0]] + list(c["costs"][1:]))
    _, q = run_entries(none)
    for a, b, what in zip(p, q, ("loss_out", "grad_rel", "grad_conn")):
        assert same_bits(a, b), what
    assert float(p[1][0].abs().max()) == 0.0       # no relation of image 0 is selected


# ------------------------------------------------------------------------------------------------------------------ model
@pytest.fixture(scope="module")
def small_model(golden_dir):
    g = Hh.load_golden(golden_dir, "sgg_small.npz")
    cfg_dict, shapes = json.loads(str(g["cfg"])), json.loads(str(g["shapes"]))
    model, cfg, sd = Hh.build_product_model(cfg_dict, shapes, int(g["seed"]))
    model.load_state_dict(sd)
    return g, model.to(DEV), cfg


def test_training_step_with_triplet_targets_equals_dense_targets(small_model, monkeypatch):
    """One training step of the small model with ``rel_triplets`` targets against the same step with dense ``rel``: every
    loss term equal exactly, every parameter gradient equal exactly, no dense target built on the packed route.

    Two separately run steps cannot be compared bit for bit: a step of this project is not bit-reproducible run to run
    (MIOpen's convolutions in the forward, float atomics in the MSDA backward: test_gpu_model.py:430, test_gpu_ddp.py:73-78),
    with whatever targets.  So both target forms are evaluated inside ONE step, on the same forward and the same matcher
    output: the criterion is called for the dense and for the triplet targets, the loss terms and the gradients it hands
    back to the four model outputs are compared bit for bit, and the step then backpropagates the element-wise
    difference of those two gradients through the one shared graph.  A parameter gradient is a linear function of the
    gradients at the model outputs, so equal parameter gradients <=> every parameter gradient of that difference is exactly
    zero: a backward pass over zeros gives zeros in any summation order -- a single differing element would not."""
    from egtr_amd import targets as T
    from egtr_amd.egtr import SceneGraphGenerationLoss
    g, model, cfg = small_model
    model.train()
    pv, pm = Hh.small_inputs(g)
    pv, pm = pv.to(DEV), pm.to(DEV)
    host = W.make_targets(int(g["target_seed"]), 2, cfg.num_queries, cfg.num_labels, cfg.num_rel_labels)
    dense = [{k: v.to(DEV) for k, v in t.items()} for t in host]
    trip = []
    for t in host:
        rows = t["rel"].nonzero()
        rows = torch.cat([rows.flip(0), rows[:1]])             # another order, one duplicate; on the HOST, as a loader gives them
        trip.append({"class_labels": t["class_labels"].to(DEV), "boxes": t["boxes"].to(DEV), "rel_triplets": rows})

    def no_dense_target(*args, **kw):
        raise AssertionError("the packed route must not materialise a dense [N, N, R] target")

    def step(targets):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(0)
        out = model(pixel_values=pv, pixel_mask=pm, labels=targets, output_attentions=False,
                    output_attention_states=True, output_hidden_states=True)
        out.loss.backward()
        torch.cuda.synchronize()
        return out, {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters() if p.grad is not None}

    # the plain step with each form (the triplet one with unpack_relations made to raise): same terms, finite, gradients everywhere
    out_d, grads_d = step(dense)
    with monkeypatch.context() as m:
        m.setattr(T, "unpack_relations", no_dense_target)
        out_t, grads_t = step(trip)
    assert set(out_d.loss_dict) == set(out_t.loss_dict) and {"loss_rel", "loss_connectivity", "uncertainty"} <= set(out_d.loss_dict)
    assert bool(torch.isfinite(out_d.loss)) and bool(torch.isfinite(out_t.loss))
    assert set(grads_d) == set(grads_t) and len(grads_d) > 10
    assert all(float(v.abs().max()) > 0 for v in grads_d.values()) and all(float(v.abs().max()) > 0 for v in grads_t.values())

    # both forms inside one step
    seen = {}
    orig_forward = SceneGraphGenerationLoss.forward
    keys = ("logits", "pred_boxes", "pred_rel", "pred_connectivity")

    def both_forms(self, outputs, targets, matched=None):
        assert targets is dense
        res, boundary = {}, {}
        for name, tg in (("dense", dense), ("trip", trip)):
            with monkeypatch.context() as m:
                if name == "trip":
                    m.setattr(T, "unpack_relations", no_dense_target)
                res[name] = orig_forward(self, outputs, tg, matched)
            total = sum(v for v in res[name].values() if v.requires_grad)
            boundary[name] = torch.autograd.grad(total, [outputs[k] for k in keys], retain_graph=True)
        seen.update(res=res, boundary=boundary)
        # the step's loss: sum_k <output_k, d trip / d output_k - d dense / d output_k> (the difference formed per element, so
        # that equal gradients cancel exactly whatever order autograd adds the terms in)
        diff = sum((outputs[k] * (t - d)).sum() for k, d, t in zip(keys, boundary["dense"], boundary["trip"]))
        out = {k: v.detach() * 0 for k, v in res["dense"].items()}
        out["loss_ce"] = diff
        return out

    with monkeypatch.context() as m:
        m.setattr(SceneGraphGenerationLoss, "forward", both_forms)
        out_z, grads_z = step(dense)
    res, boundary = seen["res"], seen["boundary"]
    assert set(res["dense"]) == set(res["trip"]) <= set(out_d.loss_dict)
    for k in res["dense"]:
        assert same_bits(res["dense"][k].detach().cpu().reshape(1), res["trip"][k].detach().cpu().reshape(1)), k
    for k, a, b in zip(keys, boundary["dense"], boundary["trip"]):
        assert same_bits(a.cpu(), b.cpu()), k
        assert float(a.abs().max()) > 0, k
    assert float(out_z.loss) == 0.0
    assert set(grads_z) == set(grads_d)
    for n, v in grads_z.items():
        assert float(v.abs().max()) == 0.0, n          # parameter gradient (triplets) - parameter gradient (dense), exactly


def test_evaluate_with_triplet_targets_equals_dense_targets(small_model):
    from egtr_amd.evaluation import evaluate
    g, model, cfg = small_model
    model.eval()
    pv, pm = Hh.small_inputs(g)
    with torch.no_grad():
        out = model(pixel_values=pv.to(DEV), pixel_mask=pm.to(DEV), output_attentions=False,
                    output_attention_states=True, output_hidden_states=True)
    C, R = cfg.num_labels, cfg.num_rel_labels
    logits, boxes, pred_rel = out["logits"].cpu(), out["pred_boxes"].cpu(), out["pred_rel"].cpu()
    sizes = torch.tensor([[480, 640], [300, 500]])
    batches = {"dense": [], "trip": []}
    for shift in (1, 2):                       # two batches with different relations, built from the model's own predictions
        dense, trip = [], []
        for b in range(2):
            n = 6
            rel = torch.zeros(n, n, R)
            for i in range(n):
                rel[i, (i + shift) % n, (i * 3) % R] = 1
                rel[i, (i + shift + 1) % n, int(pred_rel[b, i, (i + shift + 1) % n].argmax())] = 1
            base = {"class_labels": logits[b, :n, :C].argmax(-1), "boxes": boxes[b, :n], "orig_size": sizes[b]}
            rows = rel.nonzero()
            dense.append(dict(base, rel=rel))
            trip.append(dict(base, rel_triplets=torch.cat([rows.flip(0), rows[:2]])))
        batches["dense"].append({"pixel_values": pv, "pixel_mask": pm, "labels": dense})
        batches["trip"].append({"pixel_values": pv, "pixel_mask": pm, "labels": trip})
    want = evaluate(model, batches["dense"], C, R, single=True, multiple=True, graphed=False)
    got = evaluate(model, batches["trip"], C, R, single=True, multiple=True, graphed=False)
    assert set(got) == set(want) and len(want) == 12
    for k, v in want.items():
        assert got[k] == v or (v != v and got[k] != got[k]), (k, got[k], v)
    assert want["(single)R@100"] > 0
