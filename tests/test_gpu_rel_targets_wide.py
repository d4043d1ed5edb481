"""GPU (-m gpu): wide packed relation targets -- int64 [B, N, N, W] words, W = ceil(R / 64), 65 .. 256
predicates: the pack kernel against the CPU composition; the loss entries on wide words, under both tie rules and un-sampled,
bit-identical to the dense target format on the dense form of the same targets; at W = 1 bit-identical to the narrow packed
format; the float64 oracle; and the 100-predicate small model with both target forms inside ONE step (training, validation and
deterministic mode) with every dense materialisation made to raise.  The method, and the helpers ``distinct_logits``,
``matcher_flat`` and ``same_bits``, are those of tests/test_gpu_rel_targets.py."""
import functools

import numpy as np
import pytest
import torch

import loss_restated as LR
import relation_loss_all_restated as RA
import test_gpu_rel_targets as RT
import wide_model_cases as WM
from oracle import loss as OL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_SAMPLE = 80
NM = float(OL.nonmatching_cost(2.0, 5.0, 2.0, 1e-14))
OUT = ("loss_out", "grad_rel", "grad_conn")

# (N, R, per-image (targets, triplets drawn)): image 0 carries a duplicate, two predicates of ONE pair on both sides of the last
# word boundary and predicate R - 1; image 1 has targets and no relation; image 2 no target at all (T = 0).  The fourth image of
# the last case: 6 true relations in a 2 x 2 block of 100 predicates -- 80 n_true = 480 exceeds its 394 false candidates.
CASES = {
    "n7r65": (7, 65, ((5, 8), (3, 0), (0, 0))),
    "n9r100": (9, 100, ((6, 8), (4, 0), (0, 0))),
    "n6r128": (6, 128, ((4, 7), (3, 0), (0, 0))),
    "n6r129": (6, 129, ((4, 7), (3, 0), (0, 0))),
    "n5r192": (5, 192, ((4, 6), (2, 0), (0, 0))),
    "n5r193": (5, 193, ((4, 6), (2, 0), (0, 0))),
    "n5r256": (5, 256, ((4, 6), (2, 0), (0, 0))),
    "n9r100-capped": (9, 100, ((6, 8), (4, 0), (0, 0), (2, -1))),
}
BASE = tuple(n for n in CASES if n != "n9r100-capped")
CAPPED_ROWS = [[0, 1, 63], [0, 1, 64], [1, 0, 99], [0, 0, 5], [1, 1, 70], [1, 0, 0]]


def boundary(R):
    """the first predicate of the last word"""
    return 64 * ((R + 63) // 64 - 1)


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs of one case (host), built once and left unchanged."""
    N, R, images = CASES[name]
    g = torch.Generator().manual_seed(3000 + N + R + len(images))
    B = len(images)
    trips, indices, costs = [], [], []
    for T, K in images:
        if K > 0:
            so = torch.stack([torch.randint(0, T, (K,), generator=g), torch.randint(0, T, (K,), generator=g)], 1)
            t = torch.cat([so, torch.randint(0, R, (K, 1), generator=g)], 1)
            t[1] = t[0]                                              # a duplicated triplet
            t[2, :2], t[2, 2] = t[0, :2], boundary(R) - 1            # two predicates of one pair, the last bit of a word ...
            t[3, :2], t[3, 2] = t[0, :2], boundary(R)                # ... and the first bit of the next
            t[4, 2] = R - 1                                          # the top valid bit of the last word
        elif K < 0:
            t = torch.tensor(CAPPED_ROWS)
        else:
            t = torch.zeros(0, 3, dtype=torch.int64)
        trips.append(t)
        indices.append((torch.randperm(N, generator=g)[:T].sort()[0], torch.randperm(T, generator=g)))
        costs.append(torch.randn(T, generator=g) * 3)
    pred_rel = RT.distinct_logits(g, B, N, N, R)
    for b in range(B):
        assert pred_rel[b].unique().numel() == N * N * R             # no two logits of an image are equal
    pred_conn = torch.randn(B, N, N, 1, generator=g)
    dense = [RT.dense_reference_way(t, N, R) for t in trips]
    return dict(N=N, R=R, B=B, trips=trips, dense=dense, indices=indices, costs=costs, pred_rel=pred_rel, pred_conn=pred_conn)


def operands(c, indices=None):
    from egtr_amd import targets as T
    pr, pc = c["pred_rel"].to(DEV), c["pred_conn"].to(DEV)
    flat = RT.matcher_flat(indices if indices is not None else c["indices"], c["costs"])
    rels = [d.contiguous().to(DEV) for d in c["dense"]]
    ptrs = torch.tensor([r.data_ptr() for r in rels], dtype=torch.int64).to(DEV)
    words = T.pack_relations_wide([{"rel_triplets": t} for t in c["trips"]], c["N"], c["R"], DEV)
    assert tuple(words.shape) == (c["B"], c["N"], c["N"], (c["R"] + 63) // 64)
    return pr, pc, flat, rels, ptrs, words


def run_entries(c, indices=None, k=K_SAMPLE, det=False, nm=NM):
    """(dense entry, wide entry) -> (loss [2], grad_rel, grad_conn) each, same matcher outputs."""
    from egtr_amd import ops
    pr, pc, (pi, ti, mc, off), rels, ptrs, words = operands(c, indices)
    d = ops.relation_loss_launch(pr, pc, ptrs, False, pi, ti, mc, off, nm, k, k, deterministic=det)
    p = ops.relation_loss_launch(pr, pc, words, True, pi, ti, mc, off, nm, k, k, deterministic=det)
    torch.cuda.synchronize()
    del rels
    return [x.cpu() for x in d], [x.cpu() for x in p]


def run_all_entries(c, nm, want_grad, indices=None):
    from egtr_amd import ops
    pr, pc, (pi, ti, mc, off), rels, ptrs, words = operands(c, indices)
    d = ops.relation_loss_all_launch(pr, pc, ptrs, False, pi, ti, mc, off, nm, want_grad=want_grad)
    p = ops.relation_loss_all_launch(pr, pc, words, True, pi, ti, mc, off, nm, want_grad=want_grad)
    torch.cuda.synchronize()
    del rels
    return [None if x is None else x.cpu() for x in d], [None if x is None else x.cpu() for x in p]


def assert_same(d, p):
    for a, b, what in zip(d, p, OUT):
        assert (a is None) == (b is None), what
        assert a is None or RT.same_bits(a, b), what


# ---------------------------------------------------------------------------------------------------------- 1. pack kernel
@pytest.mark.parametrize("name", BASE)
def test_pack_kernel_equals_cpu_composition(name):
    from egtr_amd import targets as T
    c = case(name)
    N, R = c["N"], c["R"]
    want = T.pack_relations_wide([{"rel_triplets": t} for t in c["trips"]], N, R, "cpu")
    for b in range(c["B"]):
        assert torch.equal(T.unpack_relations(want, b, R), c["dense"][b])
    host = T.pack_relations_wide([{"rel_triplets": t} for t in c["trips"]], N, R, DEV)           # one pinned copy
    dev = T.pack_relations_wide([{"rel_triplets": t.to(DEV)} for t in c["trips"]], N, R, DEV)    # triplets already on the device
    assert host.dtype == torch.int64 and tuple(host.shape) == (c["B"], N, N, (R + 63) // 64) and host.is_contiguous()
    assert torch.equal(host.cpu(), want) and torch.equal(dev.cpu(), want)
    s, o = c["trips"][0][0, :2].tolist()
    b0 = boundary(R)
    assert int(want[0, s, o, (b0 - 1) >> 6]) < 0 and int(want[0, s, o, b0 >> 6]) & 1 == 1       # bit 63 | bit 0 of the next word
    s, o, _ = c["trips"][0][4].tolist()
    assert (int(want[0, s, o, (R - 1) >> 6]) >> ((R - 1) & 63)) & 1 == 1
    for b in range(c["B"]):
        assert torch.equal(T.unpack_relations(host, b, R).cpu(), c["dense"][b])                  # the device unpack, 4-D words


@pytest.mark.parametrize("name", BASE)
def test_pack_kernel_drops_out_of_range_device_triplets(name):
    from egtr_amd import targets as T
    c = case(name)
    N, R = c["N"], c["R"]
    good = c["trips"][0]
    bad = torch.tensor([[N, 0, 0], [0, N, 0], [0, 0, R], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [N - 1, N - 1, R], [N - 1, N - 1, 256],
                        [2 ** 40, 1, 1], [1, 2 ** 40, 1], [1, 1, 2 ** 40], [1, 1, 64 * ((R + 63) // 64)]])
    mixed = torch.cat([good[:2], bad[:4], good[2:], bad[4:]])
    tg = [{"rel_triplets": mixed.to(DEV)}, {"rel_triplets": bad.to(DEV)}, {"rel_triplets": good.to(DEV)}]
    got = T.pack_relations_wide(tg, N, R, DEV).cpu()
    want = T.pack_relations_wide([{"rel_triplets": good}, {"rel_triplets": good[:0]}, {"rel_triplets": good}], N, R, "cpu")
    assert torch.equal(got, want)
    assert int((got[1] != 0).sum()) == 0


# ------------------------------------------------------------------------------------------------------- 2. sampled entry
@pytest.mark.parametrize("name", list(CASES))
def test_wide_loss_entry_is_bit_identical_to_dense_entry(name):
    d, p = run_entries(case(name))
    assert torch.isfinite(d[0]).all()
    assert_same(d, p)
    assert int((d[1] != 0).sum()) > 0


def test_selection_bounds():
    """80 n_true against the number of false candidates of the matched block (egtr:852-858): image 3 is capped by its
    candidates (T T R - n_true, what ``count_block``'s mask gives), image 0 is not; the gradient's support has exactly the
    predicted number of elements."""
    c = case("n9r100-capped")
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
    assert capped == [False, False, False, True]
    b3 = c["dense"][3][c["indices"][3][1]][:, c["indices"][3][1]]
    assert int((b3 != 0).sum()) == 6 and int((b3 != 1).sum()) == 2 * 2 * R - 6 == 394 < K_SAMPLE * 6
    _, p = run_entries(c)
    # every selected element has a non-zero gradient (sigmoid(x) - y = 0 needs y = sigmoid(x) exactly)
    assert int((p[1] != 0).sum()) == n_sel
    assert int((p[1][3] != 0).sum()) == 6 + 394 + K_SAMPLE * 6


# ------------------------------------------------------------------------------------------------- 3. deterministic entry
@pytest.mark.parametrize("name", list(CASES))
def test_wide_deterministic_entry_is_bit_identical_to_dense_entry(name):
    d, p = run_entries(case(name), det=True)
    assert torch.isfinite(d[0]).all()
    assert_same(d, p)
    assert int((d[1] != 0).sum()) > 0


@functools.lru_cache(maxsize=None)
def tie_case():
    """The tie inputs of tests/test_gpu_deterministic.py (B = 2, N = 24, logits from {-0.5, 0, 0.5}, two per true relation
    wanted) at R = 100: far more candidates share the threshold logit than are needed."""
    B, N, R = 2, 24, 100
    g = torch.Generator().manual_seed(2024)
    pred_rel = (torch.randint(0, 3, (B, N, N, R), generator=g).float() - 1.0) * 0.5
    pred_conn = torch.randn(B, N, N, 1, generator=g)
    trips, indices, costs = [], [], []
    for T, K in ((6, 4), (5, 3)):
        so = torch.stack([torch.randint(0, T, (K,), generator=g), torch.randint(0, T, (K,), generator=g)], 1)
        t = torch.cat([so, torch.randint(0, R, (K, 1), generator=g)], 1)
        t[0, 2], t[1, 2] = 63, R - 1
        trips.append(t)
        indices.append((torch.randperm(N, generator=g)[:T].sort()[0], torch.randperm(T, generator=g)))
        costs.append(torch.randn(T, generator=g) * 3)
    dense = [RT.dense_reference_way(t, N, R) for t in trips]
    return dict(B=B, N=N, R=R, pred_rel=pred_rel, pred_conn=pred_conn, trips=trips, indices=indices, costs=costs, dense=dense)


def test_wide_deterministic_entry_where_most_candidates_tie():
    c = tie_case()
    e = LR.relation_expectation(c, 2, 2, order="key")
    for info in e.info:                        # both problems of both images: more tied candidates than needed
        for k, tied, need in info:
            assert k > 0 and 0 < need < tied, e.info
    d, p = run_entries(c, k=2, det=True)
    assert_same(d, p)
    assert np.array_equal(p[1].numpy() != 0, e.mult > 0)                    # the lowest flat index first
    d2, p2 = run_entries(c, k=2, det=True)
    assert_same(p, p2)


# ---------------------------------------------------------------------------------------------------- 4. un-sampled entry
ALL_CASES = {"n7r65": (7, 65), "n5r128": (5, 128), "n5r129": (5, 129), "n5r256": (5, 256)}


@functools.lru_cache(maxsize=None)
def all_case(name):
    """``loss_restated.build_case``: three images (some queries matched, none, all), ~5 % of ALL (row, column, predicate) set --
    also in the rows that unmatched queries take, which show in y under a non-matching cost of 0.  N R is no multiple of 256
    (455, 640, 645) except at R = 256, where every N R is one."""
    N, R = ALL_CASES[name]
    assert (N * R) % 256 != 0 or R == 256
    rng = np.random.default_rng(7000 + N + R)
    images = []
    for T in (3, 0, N):
        t = rng.random((N, N, R)) < 0.05
        t[0, 1, 63] = t[0, 1, 64] = t[N - 1, N - 1, R - 1] = True
        images.append((rng.permutation(N)[:T], rng.permutation(T), np.argwhere(t)))
    return LR.build_case(rng, rng.standard_normal((3, N, N, R)).astype(np.float32), images)


@pytest.mark.parametrize("nm", [RA.NM_COST, RA.NM_HALF])
@pytest.mark.parametrize("name", list(ALL_CASES))
def test_wide_unsampled_entry_is_bit_identical_to_dense_entry(name, nm):
    c = all_case(name)
    d, p = run_all_entries(c, nm, True)
    assert torch.isfinite(d[0]).all() and float(d[1].abs().max()) > 0
    assert_same(d, p)
    dv, pv = run_all_entries(c, nm, False)                                   # value-only: both gradients NULL
    assert pv[1] is None and pv[2] is None
    assert_same(dv, pv)
    assert RT.same_bits(pv[0], p[0])
    if nm == RA.NM_HALF:                       # the rows of unmatched queries are felt: another loss than under the constant
        other = run_all_entries(c, RA.NM_COST, False)[1][0]
        assert not RT.same_bits(other, pv[0])


# ----------------------------------------------------------------------------------------------------------------- 5. W = 1
@pytest.mark.parametrize("name", ["n7r5", "n33r64"])
def test_one_word_per_pair_equals_the_narrow_entries(name):
    from egtr_amd import ops, targets as T
    c = RT.case(name)
    N, R = c["N"], c["R"]
    tg = [{"rel_triplets": t} for t in c["trips"]]
    bits = T.pack_relations(tg, N, R, DEV)
    words = T.pack_relations_wide(tg, N, R, DEV)
    assert tuple(words.shape) == (c["B"], N, N, 1) and torch.equal(words, bits[..., None])
    pr, pc = c["pred_rel"].to(DEV), c["pred_conn"].to(DEV)
    pi, ti, mc, off = RT.matcher_flat(c["indices"], c["costs"])
    for det in (False, True):
        a = ops.relation_loss_launch(pr, pc, bits, True, pi, ti, mc, off, NM, K_SAMPLE, K_SAMPLE, deterministic=det)
        b = ops.relation_loss_launch(pr, pc, words, True, pi, ti, mc, off, NM, K_SAMPLE, K_SAMPLE, deterministic=det)
        assert_same([x.cpu() for x in a], [x.cpu() for x in b])
    for want_grad in (True, False):
        a = ops.relation_loss_all_launch(pr, pc, bits, True, pi, ti, mc, off, NM, want_grad=want_grad)
        b = ops.relation_loss_all_launch(pr, pc, words, True, pi, ti, mc, off, NM, want_grad=want_grad)
        assert_same([None if x is None else x.cpu() for x in a], [None if x is None else x.cpu() for x in b])


def test_word_count_must_match_the_predicates():
    from egtr_amd import ops
    c = case("n9r100")
    pr, pc, (pi, ti, mc, off), rels, ptrs, words = operands(c)
    for bad in (words[..., :1].contiguous(), torch.cat([words, words], -1)):
        with pytest.raises(RuntimeError, match="wide rel_bits"):
            ops.relation_loss_launch(pr, pc, bad, True, pi, ti, mc, off, NM, K_SAMPLE, K_SAMPLE)
        with pytest.raises(RuntimeError, match="wide rel_bits"):
            ops.relation_loss_all_launch(pr, pc, bad, True, pi, ti, mc, off, NM)


# ------------------------------------------------------------------------------------------------------- 6. refused image
@pytest.mark.parametrize("name", ["n7r65", "n9r100-capped"])
def test_invalid_matcher_output_is_an_image_without_matches(name):
    """-1 indices (a cost matrix the matcher refused) for image 0: the wide entries do what the dense entries do, and give what
    the same batch gives when that image has no matches at all."""
    c = case(name)
    a0, b0 = c["indices"][0]
    minus = [(torch.full_like(a0, -1), torch.full_like(b0, -1))] + list(c["indices"][1:])
    none = dict(c, indices=[(a0[:0], b0[:0])] + list(c["indices"][1:]), costs=[c["costs"][0][:0]] + list(c["costs"][1:]))
    for det in (False, True):
        d, p = run_entries(c, minus, det=det)
        assert_same(d, p)
        _, q = run_entries(none, det=det)
        assert_same(p, q)
        assert float(p[1][0].abs().max()) == 0.0       # no relation of image 0 is selected
    d, p = run_all_entries(c, NM, True, minus)
    assert_same(d, p)
    _, q = run_all_entries(none, NM, True)
    assert_same(p, q)


# ------------------------------------------------------------------------------------------------------ 7. float64 oracle
def test_wide_route_vs_oracle():
    """ops.relation_losses on ``rel_triplets`` targets at (N, R) = (9, 100) against oracle.loss.relation_losses in float64 under
    autograd: value 1e-5 relative, gradient 1e-7 absolute (the bounds of test_packed_route_vs_oracle)."""
    from egtr_amd import ops, targets as T
    c = case("n9r100")
    nm_cost = OL.nonmatching_cost(2.0, 5.0, 2.0, 1e-14)
    pr64 = c["pred_rel"].double().requires_grad_(True)
    pc64 = c["pred_conn"].double().requires_grad_(True)
    w_rel, w_conn = OL.relation_losses(pr64, pc64, [{"rel": d.double()} for d in c["dense"]], c["indices"],
                                       [x.double() for x in c["costs"]], nm_cost, K_SAMPLE, K_SAMPLE, True)
    assert not bool(torch.isnan(w_rel))
    (w_rel * 1.5 + w_conn * 0.5).backward()
    prd = c["pred_rel"].to(DEV).requires_grad_(True)
    pcd = c["pred_conn"].to(DEV).requires_grad_(True)
    packs = []
    orig = T.pack_relations_wide
    T.pack_relations_wide = lambda *a, **k: (packs.append(1), orig(*a, **k))[1]
    try:
        l_rel, l_conn = ops.relation_losses(prd, pcd, [{"rel_triplets": t} for t in c["trips"]],
                                            [(a.to(DEV), b.to(DEV)) for a, b in c["indices"]],
                                            [x.to(DEV) for x in c["costs"]], float(nm_cost), K_SAMPLE, K_SAMPLE)
    finally:
        T.pack_relations_wide = orig
    assert packs == [1]
    got_rel, want_rel, got_conn, want_conn = (float(v.detach()) for v in (l_rel, w_rel, l_conn, w_conn))
    print("loss_rel", got_rel, want_rel, "loss_conn", got_conn, want_conn)
    assert abs(got_conn - want_conn) < 1e-5 * max(1.0, abs(want_conn))
    assert abs(got_rel - want_rel) < 1e-5 * max(1.0, abs(want_rel))
    (l_rel * 1.5 + l_conn * 0.5).backward()
    e_rel, e_conn = (prd.grad.cpu().double() - pr64.grad).abs().max(), (pcd.grad.cpu().double() - pc64.grad).abs().max()
    print("gradient errors", float(e_rel), float(e_conn))
    assert e_rel < 1e-7 and e_conn < 1e-7


# ----------------------------------------------------------------------------------------------------------- 8. model level
@pytest.fixture(scope="module")
def wide_model(golden_dir):
    return WM.load(golden_dir, DEV)


def _both_target_forms(g, cfg):
    dense = WM.targets_of(g, cfg, DEV)
    trip = []
    for t in dense:
        rows = t["rel"].nonzero().cpu()
        rows = torch.cat([rows.flip(0), rows[:1]])       # another order, one duplicate; on the HOST, as a loader gives them
        trip.append({"class_labels": t["class_labels"], "boxes": t["boxes"], "rel_triplets": rows})
    assert any(int(t["rel_triplets"][:, 2].max()) >= 64 for t in trip)     # predicates of the second word
    return dense, trip


def _no_dense_target(*args, **kw):
    raise AssertionError("the wide packed route must not materialise a dense [N, N, R] target")


def _leaves(outputs):
    keys = ("logits", "pred_boxes", "pred_rel", "pred_connectivity")
    sets = [outputs] + list(outputs.get("auxiliary_outputs", []))
    return [s[k] for s in sets for k in keys if k in s and torch.is_tensor(s[k]) and s[k].requires_grad]


def _one_step_with_both_forms(wide_model, monkeypatch, train):
    """Both target forms inside ONE step, on the same forward: see test_training_step_with_triplet_targets_equals_dense_targets
    (tests/test_gpu_rel_targets.py) -- two separately run steps are not bit-reproducible.  Returns what the criterion saw and,
    in training mode, the parameter gradients of the DIFFERENCE of the two boundary gradients."""
    from egtr_amd import targets as T
    from egtr_amd.egtr import SceneGraphGenerationLoss
    g, model, cfg, pv, pm = wide_model
    assert cfg.num_rel_labels == 100
    dense, trip = _both_target_forms(g, cfg)
    seen = {"packs": 0}
    orig_forward = SceneGraphGenerationLoss.forward
    orig_pack = T.pack_relations_wide

    def counted_pack(*a, **k):
        seen["packs"] += 1
        return orig_pack(*a, **k)

    def both_forms(self, outputs, targets, matched=None):
        assert targets is dense and self.model_training is train
        res, bound = {}, {}
        leaves = _leaves(outputs) if train else []
        for name, tg in (("dense", dense), ("trip", trip)):
            with monkeypatch.context() as m:
                if name == "trip":
                    m.setattr(T, "materialize_relations", _no_dense_target)
                    m.setattr(T, "unpack_relations", _no_dense_target)
                    m.setattr(T, "pack_relations_wide", counted_pack)
                res[name] = dict(orig_forward(self, outputs, tg, matched))
            if train:
                total = sum(v for v in res[name].values() if v.requires_grad)
                grads = torch.autograd.grad(total, leaves, retain_graph=True, allow_unused=True)
                bound[name] = [torch.zeros_like(x) if gr is None else gr for x, gr in zip(leaves, grads)]
        seen.update(res=res, bound=bound)
        if not train:
            return dict(res["trip"])           # (the model adds its own entries to the dict it gets back)
        diff = sum((x * (t - d)).sum() for x, d, t in zip(leaves, bound["dense"], bound["trip"]))
        out = {k: v.detach() * 0 for k, v in res["dense"].items()}
        out["loss_ce"] = diff
        return out

    grads = None
    with monkeypatch.context() as m:
        m.setattr(SceneGraphGenerationLoss, "forward", both_forms)
        if train:
            model.train()
            model.zero_grad(set_to_none=True)
            out = model(pixel_values=pv, pixel_mask=pm, labels=dense, output_attention_states=True)
            out.loss.backward()
            torch.cuda.synchronize()
            grads = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters() if p.grad is not None}
            model.zero_grad(set_to_none=True)
            model.eval()
        else:
            model.eval()
            with torch.no_grad():
                out = model(pixel_values=pv, pixel_mask=pm, labels=dense, output_attention_states=True)
            torch.cuda.synchronize()
    res = seen["res"]
    assert seen["packs"] == 1                                          # packed wide, once for the step: both terms share the words
    assert set(res["dense"]) == set(res["trip"]) and {"loss_rel", "loss_connectivity", "uncertainty"} <= set(res["dense"])
    assert any(k.endswith("_0") for k in res["dense"])               # the auxiliary terms
    for k in res["dense"]:
        a, b = res["dense"][k].detach().float().cpu().reshape(1), res["trip"][k].detach().float().cpu().reshape(1)
        assert bool(torch.isfinite(a).all()), k
        assert RT.same_bits(a, b), k
    return out, seen, grads


def _check_training_step(out, seen, grads):
    assert len(seen["bound"]["dense"]) >= 4
    for a, b in zip(seen["bound"]["dense"], seen["bound"]["trip"]):
        assert RT.same_bits(a.cpu(), b.cpu())
    assert sum(float(a.abs().max()) > 0 for a in seen["bound"]["dense"]) >= 4
    assert float(out.loss) == 0.0
    assert len(grads) > 10
    for n, v in grads.items():
        assert float(v.abs().max()) == 0.0, n          # parameter gradient (triplets) - parameter gradient (dense), exactly


def test_training_step_with_triplet_targets_equals_dense_targets_at_100_predicates(wide_model, monkeypatch):
    _check_training_step(*_one_step_with_both_forms(wide_model, monkeypatch, True))


def test_validation_forward_with_triplet_targets_equals_dense_targets_at_100_predicates(wide_model, monkeypatch):
    """evaluation mode under ``no_grad``: the un-sampled, value-only route reads the words"""
    out, seen, _ = _one_step_with_both_forms(wide_model, monkeypatch, False)
    assert bool(torch.isfinite(out.loss)) and not out.loss.requires_grad


def test_deterministic_training_step_with_triplet_targets_equals_dense_targets_at_100_predicates(wide_model, monkeypatch):
    from egtr_amd import ops
    with ops.deterministic():
        res = _one_step_with_both_forms(wide_model, monkeypatch, True)
    _check_training_step(*res)
