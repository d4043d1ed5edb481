"""GPU (-m gpu): the relation loss's selection (csrc/loss.hip: prep, 3-pass radix select, tie count, final pass) at the edges the
smooth-logit tests never reach -- ties that span steps, waves and more than 256 rows; N > 1024; logits that share one radix bin,
22 leading bits, a sign, or sit at +-0 / denormals; k = 1 and k = everything; images without matches or relations; dense targets
that are not 0 / 1.  Inputs and the float64 expectation: tests/loss_restated.py (its preconditions: tests/test_loss_cases_cpu.py).

Bars (the existing ones of test_relation_loss_kernel_vs_oracle, with a relative term for selections of a handful of elements,
where one gradient is ~0.3 and four fp32 roundings exceed 1e-7): loss 1e-5 relative, gradient max(1e-7, 1e-6 max|grad_ref|).
Largest errors observed on an MI355X (each test prints its own under -s): gradient 1.7e-8 at a bar of 1.5e-7 (radix families,
k = 1), 1e-8 at 1e-7 elsewhere, 2e-12 in the large tied cases; loss 8.8e-8 relative."""
import numpy as np
import pytest
import torch

import loss_restated as LR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_BAR = 1e-5


def launch(c, k_neg, k_nm, packed, det):
    """ops.relation_loss_launch on a case -> (loss [2], grad_rel, grad_conn) on the host."""
    import test_gpu_rel_targets as RT
    from egtr_amd import ops, targets as T
    pr, pc = c["pred_rel"].to(DEV), c["pred_conn"].to(DEV)
    pi, ti, mc, off = RT.matcher_flat(c["indices"], c["costs"])
    if packed:
        target = keep = T.pack_relations([{"rel_triplets": t} for t in c["trips"]], c["N"], c["R"], DEV)
    else:
        keep = [d.contiguous().to(DEV) for d in c["dense"]]
        target = torch.tensor([r.data_ptr() for r in keep], dtype=torch.int64).to(DEV)
    out = ops.relation_loss_launch(pr, pc, target, packed, pi, ti, mc, off, LR.NM_COST, k_neg, k_nm, deterministic=det)
    torch.cuda.synchronize()
    del keep
    return [t.cpu() for t in out]


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def grad_bar(ref):
    return max(1e-7, 1e-6 * float(np.abs(ref).max()))


def rel_err(got, want):
    return abs(got - want) / abs(want)


def check_deterministic(e, out, tag):
    """grad != 0 <=> mult > 0 exactly; gradient and loss within the bars of the key-order expectation."""
    loss, g = float(out[0][0]), out[1].double().numpy()
    assert np.array_equal(g != 0, e.mult > 0), tag
    err, bar, lerr = float(np.abs(g - e.grad).max()), grad_bar(e.grad), rel_err(loss, e.loss_rel)
    print(f"{tag}: grad err {err:.3e} (bar {bar:.3e}), loss rel err {lerr:.3e} (bar {LOSS_BAR:.0e})")
    assert err < bar and lerr < LOSS_BAR, tag
    return err / bar, lerr


def check_ticket(e, out, tag):
    """What holds for ANY valid choice among the candidates tied at the threshold (0 / 1 targets: an element enters once)."""
    assert int(e.mult.max()) <= 1
    loss, g = float(out[0][0]), out[1].double().numpy()
    sel = g != 0
    for b, s in enumerate(e.images):
        true = (s.mult - s.sel[0] - s.sel[1]) > 0
        assert sel[b][true].all(), tag                                    # every true relation of the block
        for prob in range(2):
            below = s.cand[prob] & ~s.above[prob] & ~s.tied[prob]
            assert sel[b][s.above[prob]].all(), (tag, b, prob)            # above the threshold: selected
            assert not sel[b][below].any(), (tag, b, prob)                # below: never
            assert int(sel[b][s.tied[prob]].sum()) == s.info[prob][2], (tag, b, prob, s.info)   # at it: exactly `need`
    assert int(sel.sum()) == e.total, tag                                 # ... and nothing else
    err, bar, lerr = float(np.abs(g - sel * e.unit).max()), grad_bar(e.grad), rel_err(loss, e.loss_rel)
    print(f"{tag}: grad err {err:.3e} (bar {bar:.3e}), loss rel err {lerr:.3e} (bar {LOSS_BAR:.0e})")
    assert err < bar and lerr < LOSS_BAR, tag
    return err / bar, lerr


def unique_selection(e):
    return all(need == tied for info in e.info for _, tied, need in info)


def check_all_routes(c, k_neg, k_nm, tag):
    """Both routes, both target forms.  Returns (expectation, the deterministic dense result, worst error / bar)."""
    e = LR.relation_expectation(c, k_neg, k_nm, "key")
    forms = (False, True) if c["trips"] is not None else (False,)
    det = {p: launch(c, k_neg, k_nm, p, True) for p in forms}
    again = launch(c, k_neg, k_nm, False, True)
    for a, b, what in zip(det[False], again, ("loss", "grad_rel", "grad_conn")):
        assert same_bits(a, b), (tag, "two runs", what)
    if True in det:
        for a, b, what in zip(det[False], det[True], ("loss", "grad_rel", "grad_conn")):
            assert same_bits(a, b), (tag, "dense / packed", what)
    worst = [check_deterministic(e, det[False], tag + " det")]
    for p in forms:
        out = launch(c, k_neg, k_nm, p, False)
        if int(e.mult.max()) <= 1:
            worst.append(check_ticket(e, out, tag + (" ticket packed" if p else " ticket dense")))
        if unique_selection(e):          # the same set, the same arithmetic
            assert same_bits(out[1], det[False][1]), (tag, "ticket route / deterministic route", p)
        assert same_bits(out[2], det[False][2]), (tag, "grad_conn", p)
    return e, det[False], (max(w[0] for w in worst), max(w[1] for w in worst))


# ------------------------------------------------------------------------------------------------------- B1 - B3: ties
@pytest.mark.parametrize("which", ["mid", "last"])
def test_ties_across_the_steps_of_a_row(which):
    """N R = 1200: the rank of a tied candidate carries the counts of the row's earlier 256-wide steps (run0 / run1) and reads
    the wave counts of the double-buffered s_wc; "last": both cuts in the fifth step, 176 live lanes."""
    c = LR.steps_case()
    e, _, worst = check_all_routes(c, *c["ks"][which], f"steps/{which}")
    assert not unique_selection(e)
    print("steps", which, "cuts (row, step, wave)", e.cuts[0], "worst err / bar, loss", worst)


def test_ties_beyond_256_rows():
    """N = 264: the cuts lie in rows >= 256 -- the prefix over the tie counts of the rows in front runs twice per thread."""
    c = LR.rows_case()
    e, _, worst = check_all_routes(c, *c["ks"]["rows"], "rows")
    assert not unique_selection(e)
    print("rows cuts (row, step, wave)", e.cuts[0], "worst err / bar, loss", worst)


def test_more_than_1024_queries():
    """N = 1030: rel_loss_prep's scan over the unmatched queries takes two chunks (the running base), matched queries and
    non-zero targets of unmatched queries beyond 1024; connectivity and loss_rel also against the oracle."""
    c = LR.scan_case()
    k_neg, k_nm = c["ks"]["scan"]
    e, det, worst = check_all_routes(c, k_neg, k_nm, "scan")
    assert not unique_selection(e)
    l_rel, l_conn, _, g_conn = LR.oracle_relation(c, k_neg, k_nm)       # its choice among ties: another valid one, same value
    assert rel_err(e.loss_rel, l_rel) < 1e-12
    loss, _, grad_conn = det
    cerr, cbar = float(np.abs(grad_conn.double().numpy() - g_conn).max()), grad_bar(g_conn)
    print(f"scan: conn grad err {cerr:.3e} (bar {cbar:.3e}), conn loss rel err {rel_err(float(loss[1]), l_conn):.3e}, "
          f"rel loss vs oracle {rel_err(float(loss[0]), l_rel):.3e}; worst err / bar, loss {worst}")
    assert cerr < cbar
    assert rel_err(float(loss[1]), l_conn) < LOSS_BAR and rel_err(float(loss[0]), l_rel) < LOSS_BAR
    assert int((g_conn < 0).sum()) == len(c["extra"]) + 1               # the pairs with a relation: target 1


# ------------------------------------------------------------------------------------------------------ B4: radix select
@pytest.mark.parametrize("family", LR.RADIX_FAMILIES)
def test_radix_select_families(family):
    """2048 logits built from bit patterns, k in {1, 2, 37, 500, everything}: one first-digit bin (passes 1 and 2 select alone),
    22 shared leading bits (pass 2 alone), complemented keys, many bins of both signs, thresholds at +-0 / denormals."""
    c = LR.radix_case(family)
    worst = []
    for k in LR.RADIX_KS:
        e, det, w = check_all_routes(c, k, k, f"radix/{family}/k={k}")
        worst.append(w)
        if family == "zeros":      # -0.0 and +0.0 have equal loss terms: the value-order expectation has the same loss
            v = LR.relation_expectation(c, k, k, "value")
            assert rel_err(float(det[0][0]), v.loss_rel) < LOSS_BAR
    print("radix", family, "worst err / bar", max(w[0] for w in worst), "worst loss rel err", max(w[1] for w in worst))


# -------------------------------------------------------------------------------------------------- B5: degenerate counts
def test_degenerate_images_in_one_batch():
    """All queries matched | no target | targets without a relation | an ordinary image with ties."""
    c = LR.degenerate_case()
    e, det, worst = check_all_routes(c, 2, 2, "degenerate")
    g = det[1]
    assert float(g[1].abs().max()) == 0.0 and float(g[2].abs().max()) == 0.0
    assert float(g[0].abs().max()) > 0 and float(g[3].abs().max()) > 0
    alone = LR.single_image(c, 3)
    ea, da, _ = check_all_routes(alone, 2, 2, "degenerate/image 3 alone")
    assert np.array_equal(ea.mult[0], e.mult[3]) and 0 < ea.total < e.total
    scaled = g[3].double().numpy() * (e.total / ea.total)
    err, bar = float(np.abs(scaled - da[1][0].double().numpy()).max()), grad_bar(ea.grad)
    print(f"degenerate: image 3 in the batch x {e.total}/{ea.total} vs alone: {err:.3e} (bar {bar:.3e}); worst {worst}")
    assert err < bar


@pytest.mark.parametrize("k_neg,k_nm", [(0, 3), (3, 0)])
def test_zero_sample_counts(k_neg, k_nm):
    """sample_negatives = 0 or sample_nonmatching = 0: the oracle's `neg == 0` branch (tie-free logits, so its selection is THE
    selection)."""
    c = LR.degenerate_case(True)
    e, det, worst = check_all_routes(c, k_neg, k_nm, f"zero/{k_neg},{k_nm}")
    assert unique_selection(e)
    l_rel, l_conn, g_rel, g_conn = LR.oracle_relation(c, k_neg, k_nm)
    err, bar = float(np.abs(det[1].double().numpy() - g_rel).max()), grad_bar(g_rel)
    print(f"zero {k_neg},{k_nm}: grad err vs oracle {err:.3e} (bar {bar:.3e}); worst {worst}")
    assert err < bar and np.array_equal(det[1].numpy() != 0, g_rel != 0)
    assert rel_err(float(det[0][0]), l_rel) < LOSS_BAR and rel_err(float(det[0][1]), l_conn) < LOSS_BAR
    assert float(np.abs(det[2].double().numpy() - g_conn).max()) < grad_bar(g_conn)


# ------------------------------------------------------------------------------------------- B6: targets that are not 0 / 1
@pytest.mark.parametrize("k", [2, 80])
def test_dense_targets_that_are_not_zero_or_one(k):
    """A block target of 0.5 or 2.0 is a true relation (!= 0) AND a false candidate (!= 1): it can enter the mean twice.  Dense
    entry only; the expectation is the oracle under autograd."""
    c = LR.nonbinary_case()
    e, det, worst = check_all_routes(c, k, k + 1, f"nonbinary/k={k}")
    assert int(e.mult.max()) == 2 and unique_selection(e)
    l_rel, l_conn, g_rel, g_conn = LR.oracle_relation(c, k, k + 1)
    err, bar = float(np.abs(det[1].double().numpy() - g_rel).max()), grad_bar(g_rel)
    print(f"nonbinary k={k}: grad err vs oracle {err:.3e} (bar {bar:.3e}); worst {worst}")
    assert err < bar and np.array_equal(det[1].numpy() != 0, g_rel != 0)
    assert rel_err(float(det[0][0]), l_rel) < LOSS_BAR and rel_err(float(det[0][1]), l_conn) < LOSS_BAR
    assert float(np.abs(det[2].double().numpy() - g_conn).max()) < grad_bar(g_conn)
