"""GPU (-m gpu): the relation loss with one sampling policy per candidate class (csrc/loss.hip, policy_neg / policy_nm of
egtr_relation_loss_f32) against the float64 twin tests/relation_sampling_restated.py (its anchors: tests/test_relation_sampling_cpu.py).

Bars, those of test_gpu_loss_selection.py: loss 1e-5 relative, gradient max(1e-7, 1e-6 max|grad_ref|), and grad != 0 <=> mult > 0
exactly -- the selected SET is the twin's, element by element.  Where a `largest` class has candidates tied at its threshold the
deterministic tie rule takes the twin's (lowest flat index first); the ticket rule may take others of the tied ones, so there the
set is compared outside them and counted inside."""
import random

import numpy as np
import pytest
import torch

import loss_restated as LR
import relation_loss_all_restated as RA
import relation_sampling_restated as RS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_BAR = 1e-5
L, Rn, A = "largest", "random", "all"
PAIRS = [(a, b) for a in (L, Rn, A) for b in (L, Rn, A) if (a, b) not in ((L, L), (A, A))]


def policy(name, count):
    return (name, None if name == A else count)


def operands(c, form):
    """(target, packed, keep-alive) of a case: "dense" pointer table, "packed" one-word or "wide" words."""
    from egtr_amd import targets as T
    if form == "dense":
        keep = [d.contiguous().to(DEV) for d in c["dense"]]
        return torch.tensor([r.data_ptr() for r in keep], dtype=torch.int64).to(DEV), False, keep
    pack = T.pack_relations_wide if form == "wide" else T.pack_relations
    bits = pack([{"rel_triplets": t} for t in c["trips"]], c["N"], c["R"], DEV)
    return bits, True, bits


def launch(c, negatives, nonmatching, seed=0, stream=0, form="dense", det=False):
    """ops.relation_loss_policy_launch on a case -> (loss [2], grad_rel, grad_conn) on the host."""
    from egtr_amd import ops
    pr, pc = c["pred_rel"].to(DEV), c["pred_conn"].to(DEV)
    pi, ti, mc, off = RA.matcher_flat(c["indices"], c["costs"], DEV)
    target, packed, keep = operands(c, form)
    out = ops.relation_loss_policy_launch(pr, pc, target, packed, pi, ti, mc, off, LR.NM_COST, negatives, nonmatching, seed,
                                          stream, deterministic=det)
    torch.cuda.synchronize()
    del keep
    return [t.cpu() for t in out]


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def grad_bar(ref):
    return max(1e-7, 1e-6 * float(np.abs(ref).max()))


def rel_err(got, want):
    return abs(got - want) / abs(want)


def check(e, out, tag, exact=True):
    """The selected set, the gradient and the loss of one launch against the expectation ``e``.  ``exact=False`` (the ticket
    entry with a tied `largest` class): outside the tied candidates the set is the twin's, inside as many are taken."""
    loss, g = float(out[0][0]), out[1].double().numpy()
    sel = g != 0
    if exact or not e.free.any():
        assert np.array_equal(sel, e.mult > 0), tag
        err = float(np.abs(g - e.grad).max())
    else:
        assert int(e.mult.max()) <= 1
        keep = ~e.free
        assert np.array_equal(sel[keep], (e.mult > 0)[keep]), tag
        assert int(sel.sum()) == e.total, tag
        err = float(np.abs(g - sel * e.unit).max())
    bar, lerr = grad_bar(e.grad), rel_err(loss, e.loss_rel)
    print(f"{tag}: grad err {err:.3e} (bar {bar:.3e}), loss rel err {lerr:.3e} (bar {LOSS_BAR:.0e})")
    assert err < bar and lerr < LOSS_BAR, tag


def check_all_routes(c, negatives, nonmatching, seed, stream, tag, forms=None):
    """Deterministic and ticket entry, every target form of the case.  Returns (expectation, the deterministic dense result)."""
    e = RS.expectation(c, negatives, nonmatching, seed, stream)
    forms = forms or (("dense", "packed") if c["trips"] is not None else ("dense",))
    det = {f: launch(c, negatives, nonmatching, seed, stream, f, True) for f in forms}
    for f in forms[1:]:
        for a, b, what in zip(det[forms[0]], det[f], ("loss", "grad_rel", "grad_conn")):
            assert same_bits(a, b), (tag, forms[0], f, what)
    check(e, det[forms[0]], tag + " det")
    for f in forms:
        out = launch(c, negatives, nonmatching, seed, stream, f, False)
        check(e, out, f"{tag} ticket {f}", exact=False)
        if not e.free.any():        # the same set, the same arithmetic
            assert same_bits(out[1], det[forms[0]][1]) and same_bits(out[0], det[forms[0]][0]), (tag, "ticket / det", f)
        assert same_bits(out[2], det[forms[0]][2]), (tag, "grad_conn", f)
    return e, det[forms[0]]


# ------------------------------------------------------------------------------------------------------------- the uniform case
def test_uniform_case_selects_the_twins_sets_for_every_image_and_stream():
    """B = 256 images x 16 launches (streams 0 .. 15), k = 8 of 26 and 8 of 81: the device's sets are the twin's -- whose
    uniformity tests/test_relation_sampling_cpu.py establishes -- in both entries and both target forms, with the same bits."""
    c = RS.uniform_case()
    seed = RS.UNIFORM_SEEDS[1]
    neg, nm = (Rn, RS.UNIFORM_KS[0][0]), (Rn, RS.UNIFORM_KS[0][1])
    sets = []
    for stream in range(RS.UNIFORM_STREAMS):
        e = RS.expectation(c, neg, nm, seed, stream)
        assert e.total == c["B"] * (1 + 8 + 8)
        outs = [launch(c, neg, nm, seed, stream, f, d) for f in ("dense", "packed") for d in (False, True)]
        outs.append(launch(c, neg, nm, seed, stream, "dense", False))       # a second run
        for o in outs:
            assert np.array_equal(o[1].numpy() != 0, e.mult > 0), stream      # every image's set
        for o in outs[1:]:
            for a, b in zip(outs[0], o):
                assert same_bits(a, b), stream
        if stream in (0, RS.UNIFORM_STREAMS - 1):
            check(e, outs[0], f"uniform/stream {stream}")
        sets.append(e.mult > 0)
    assert not any(np.array_equal(sets[0], s) for s in sets[1:])


# ------------------------------------------------------------------------------------------------------------ the policy matrix
@pytest.mark.parametrize("pair", PAIRS, ids=["-".join(p) for p in PAIRS])
def test_policy_matrix(pair):
    """Every pair of policies but (largest, largest) and (all, all), on a plain batch, on images without matches or relations
    (three-valued logits: ties in a `largest` class) and on dense targets that are not 0 / 1; counts that saturate and counts of 0."""
    for name, c in (("plain", LR.plain_case()), ("degenerate", LR.degenerate_case()), ("nonbinary", LR.nonbinary_case())):
        for k_neg, k_nm in ((2, 3), (80, 80), (0, 3), (3, 0)):
            tag = f"{pair[0]}-{pair[1]}/{name}/{k_neg},{k_nm}"
            e, det = check_all_routes(c, policy(pair[0], k_neg), policy(pair[1], k_nm), 21, 6, tag)
            if name == "degenerate":      # image 1: no match -> everything outside; image 2: matches, no relation
                g = det[1]
                assert (float(g[1].abs().max()) > 0) == (pair[1] == A), tag
                assert (float(g[2].abs().max()) > 0) == (A in pair), tag
            if name == "nonbinary" and (pair[0] == A or k_neg == 80):   # a 0.5 / 2.0 target: a true relation AND a candidate
                assert int(e.mult.max()) == 2, tag


# --------------------------------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("pair", [(Rn, Rn), (L, Rn), (Rn, A), (A, Rn)], ids=lambda p: "-".join(p))
def test_rows_of_299_elements(pair):
    """N = 23, R = 13, T = 9: a row is 299 elements -- a second, partial 256-wide step -- and R is no power of two (the flat
    index of the key is (qa N + qb) R + r)."""
    c = RS.geometry_case("odd")
    check_all_routes(c, policy(pair[0], 2), policy(pair[1], 3), 4, 9, "odd/" + "-".join(pair))


def test_tied_largest_class_beside_a_random_class_beyond_256_rows():
    """N = 260, R = 3, (largest, random) under the deterministic tie rule: the tie-count prefix runs over more than 256 rows
    and must count the block's tied candidates only -- the random class has none, whatever its logits."""
    c = RS.geometry_case("rows")
    neg, nm = (L, c["count_neg"]), (Rn, 80)
    e = RS.expectation(c, neg, nm, 8, 2)
    assert e.free.any() and not e.free[0][~np.asarray(e.images[0].cand[0])].any()     # ties decide, in the block alone
    last = np.nonzero((e.free[0] & (e.mult[0] > 0)).reshape(-1))[0][-1]
    assert LR.position(last, c["N"], c["R"])[0] >= 256                                 # ... the last one beyond row 256
    outs = {f: launch(c, neg, nm, 8, 2, f, True) for f in ("dense", "packed")}
    check(e, outs["dense"], "rows det")
    for a, b in zip(outs["dense"], outs["packed"]):
        assert same_bits(a, b)
    check(e, launch(c, neg, nm, 8, 2, "dense", False), "rows ticket", exact=False)


# ------------------------------------------------------------------------------------------------------------------- wide words
@pytest.mark.parametrize("pair", [(Rn, Rn), (A, Rn)], ids=lambda p: "-".join(p))
def test_wide_words(pair):
    """R = 70: two words per pair, predicates on both sides of bit 64."""
    c = RS.wide_case()
    check_all_routes(c, policy(pair[0], 2), policy(pair[1], 3), 13, 1, "wide/" + "-".join(pair), forms=("dense", "wide"))


# -------------------------------------------------------------------------------------------------------------- stream and seed
def test_stream_and_seed_select_other_sets_and_the_old_entries_keep_their_bits():
    from egtr_amd import ops
    c = LR.plain_case()
    neg, nm = (Rn, 2), (Rn, 3)

    def old():
        pr, pc = c["pred_rel"].to(DEV), c["pred_conn"].to(DEV)
        pi, ti, mc, off = RA.matcher_flat(c["indices"], c["costs"], DEV)
        res = []
        for form in ("dense", "packed"):
            target, packed, keep = operands(c, form)
            for det in (False, True):
                res += [t.cpu() for t in ops.relation_loss_launch(pr, pc, target, packed, pi, ti, mc, off, LR.NM_COST, 2, 3,
                                                                  deterministic=det)]
            res += [t.cpu() for t in ops.relation_loss_all_launch(pr, pc, target, packed, pi, ti, mc, off, LR.NM_COST)]
            del keep
        return res

    before = old()
    sets = {(seed, stream): launch(c, neg, nm, seed, stream)[1].numpy() != 0 for seed in (5, 6) for stream in (0, 1)}
    after = old()
    for a, b in zip(before, after):
        assert same_bits(a, b)
    for key, s in sets.items():
        assert np.array_equal(s, RS.expectation(c, neg, nm, *key).mult > 0), key
    assert not np.array_equal(sets[5, 0], sets[5, 1]) and not np.array_equal(sets[5, 0], sets[6, 0])
    # (largest, largest) through the policy entry: the set and the bits of the old deterministic entry (tie-free logits).  Both
    # sides are now the same entry with the same arguments and run the same kernel instantiation.
    pol = launch(c, (L, 2), (L, 3), det=True)
    assert same_bits(pol[1], before[4]) and same_bits(pol[2], before[5])
    assert rel_err(float(pol[0][0]), float(before[3][0])) < 1e-6


# -------------------------------------------------------------------------------------------------------------------- criterion
def criterion(c, neg, nm, neg_largest=True, nm_largest=True):
    crit = RA.criterion(c["N"], c["R"], True).to(DEV)
    crit.rel_sample_negatives, crit.rel_sample_nonmatching = neg, nm
    crit.rel_sample_negatives_largest, crit.rel_sample_nonmatching_largest = neg_largest, nm_largest
    return crit


def criterion_inputs(c, form):
    tg = ([{"rel": d.to(DEV)} for d in c["dense"]] if form == "dense" else [{"rel_triplets": t.to(DEV)} for t in c["trips"]])
    idx = [(a.to(DEV), b.to(DEV)) for a, b in c["indices"]]
    return tg, idx, [x.to(DEV) for x in c["costs"]]


def spy(monkeypatch, ops):
    calls, orig = [], ops.relation_losses_sampled

    def wrapped(*a, **k):
        calls.append(ops.relation_sampler_state())
        return orig(*a, **k)

    monkeypatch.setattr(ops, "relation_losses_sampled", wrapped)
    return calls


@pytest.mark.parametrize("form", ["dense", "triplets"])
def test_criterion_with_random_sampling_under_the_device_sampler(form, monkeypatch):
    """``*_largest=False``: under relation_sampler_mode("device", seed=5) the policy kernels evaluate the loss -- the twin's value
    at the recorded (seed, stream), one stream per call, Python's `random` untouched, the gradient scaled by the upstream
    gradient; under the default sampler the reference's composition and its random.sample draws."""
    from egtr_amd import ops
    c = LR.plain_case()
    crit = criterion(c, 2, 3, False, False)
    tg, idx, costs = criterion_inputs(c, form)
    calls = spy(monkeypatch, ops)
    state = random.getstate()
    with ops.relation_sampler_mode("device", seed=5):
        for step in range(3):
            pr = c["pred_rel"].to(DEV).requires_grad_(True)
            out = crit.loss_relations({"pred_rel": pr, "pred_connectivity": c["pred_conn"].to(DEV)}, tg, idx, costs, 1.0)
            assert calls[-1] == (5, step) and ops.relation_sampler_state() == (5, step + 1)
            e = RS.expectation(c, (Rn, 2), (Rn, 3), 5, step)
            (3.0 * out["loss_rel"]).backward()
            g = pr.grad.double().cpu().numpy()
            assert np.array_equal(g != 0, e.mult > 0), step
            assert float(np.abs(g - 3.0 * e.grad).max()) < 3.0 * grad_bar(e.grad)
            assert rel_err(float(out["loss_rel"]), e.loss_rel) < LOSS_BAR
    assert random.getstate() == state and len(calls) == 3
    draws = []
    real = random.sample
    monkeypatch.setattr(random, "sample", lambda pop, k: (draws.append(k), real(pop, k))[1])
    out = crit.loss_relations({"pred_rel": c["pred_rel"].to(DEV), "pred_connectivity": c["pred_conn"].to(DEV)}, tg, idx, costs,
                              1.0)
    assert len(calls) == 3 and draws and bool(torch.isfinite(out["loss_rel"]))      # "python": the composition drew


@pytest.mark.parametrize("counts", [(None, 80), (80, None), (None, 2), (3, None)])
@pytest.mark.parametrize("sampler", ["python", "device"])
def test_criterion_with_one_class_taken_whole(counts, sampler, monkeypatch):
    """One count None next to a `largest` class: the policy kernels under either sampler; value and gradient agree with the
    tensor composition _loss_relations_device (tie-free logits) within the bars, and with the twin."""
    from egtr_amd import ops
    c = LR.plain_case()
    crit = criterion(c, *counts)
    tg, idx, costs = criterion_inputs(c, "dense")
    calls = spy(monkeypatch, ops)
    with ops.relation_sampler_mode(sampler):
        before = ops.relation_sampler_state()
        pr = c["pred_rel"].to(DEV).requires_grad_(True)
        outputs = {"pred_rel": pr, "pred_connectivity": c["pred_conn"].to(DEV)}
        out = crit.loss_relations(outputs, tg, idx, costs, 1.0)
        assert len(calls) == 1 and ops.relation_sampler_state() == before          # no random class: no stream consumed
        g, = torch.autograd.grad(out["loss_rel"], pr)
        pr2 = c["pred_rel"].to(DEV).requires_grad_(True)
        ref = crit._loss_relations_device({"pred_rel": pr2, "pred_connectivity": c["pred_conn"].to(DEV)}, tg, idx, costs)
        g2, = torch.autograd.grad(ref["loss_rel"], pr2)
    pol = [(A, None) if k is None else (L, k) for k in counts]
    e = RS.expectation(c, pol[0], pol[1])
    g, g2 = g.double().cpu().numpy(), g2.double().cpu().numpy()
    assert np.array_equal(g != 0, e.mult > 0) and np.array_equal(g2 != 0, e.mult > 0)
    err, bar = float(np.abs(g - g2).max()), grad_bar(g2)
    print(f"{counts} {sampler}: kernels vs composition grad {err:.3e} (bar {bar:.3e}), vs twin {float(np.abs(g - e.grad).max()):.3e}")
    assert err < bar and float(np.abs(g - e.grad).max()) < grad_bar(e.grad)
    assert rel_err(float(out["loss_rel"]), float(ref["loss_rel"])) < LOSS_BAR
    assert rel_err(float(out["loss_rel"]), e.loss_rel) < LOSS_BAR
    assert rel_err(float(out["loss_connectivity"]), float(ref["loss_connectivity"])) < LOSS_BAR


def test_relation_losses_keeps_its_value_error_and_sampled_takes_explicit_streams():
    from egtr_amd import ops
    c = LR.plain_case()
    tg, idx, costs = criterion_inputs(c, "dense")
    pr, pc = c["pred_rel"].to(DEV), c["pred_conn"].to(DEV)
    with pytest.raises(ValueError):
        ops.relation_losses(pr, pc, tg, idx, costs, LR.NM_COST, None, 80)
    before = ops.relation_sampler_state()
    a = ops.relation_losses_sampled(pr, pc, tg, idx, costs, LR.NM_COST, (Rn, 2), (A, None), seed=7, stream=11)
    assert ops.relation_sampler_state() == before                                    # explicit words: the state stays
    e = RS.expectation(c, (Rn, 2), (A, None), 7, 11)
    assert rel_err(float(a[0]), e.loss_rel) < LOSS_BAR
