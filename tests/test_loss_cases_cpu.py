"""CPU: tests/loss_restated.py -- the float64 restatement of the relation loss pinned to oracle.loss.relation_losses on
tie-free inputs, the key order, and the PRECONDITIONS that give each case of tests/test_gpu_loss_selection.py its meaning
(asserted on the generated data: a changed seed cannot silently hollow a case out)."""
import numpy as np
import pytest
import torch

import loss_restated as LR


# ------------------------------------------------------------------------------------------ restatement vs the oracle
@pytest.mark.parametrize("name,k_neg,k_nm", [("plain", 3, 5), ("plain", 80, 80), ("plain", 0, 4), ("plain", 4, 0),
                                             ("nonbinary", 2, 3), ("nonbinary", 80, 80), ("degenerate", 2, 2),
                                             ("degenerate", 0, 3), ("degenerate", 3, 0)])
@pytest.mark.parametrize("order", ["value", "key"])
def test_restatement_equals_the_oracle_on_tie_free_inputs(name, k_neg, k_nm, order):
    c = {"plain": LR.plain_case, "nonbinary": LR.nonbinary_case, "degenerate": lambda: LR.degenerate_case(True)}[name]()
    for b in range(c["B"]):
        assert c["pred_rel"][b].unique().numel() == c["N"] ** 2 * c["R"]      # tie-free: one valid selection
    e = LR.relation_expectation(c, k_neg, k_nm, order)
    l_rel, _, g_rel, _ = LR.oracle_relation(c, k_neg, k_nm)
    assert e.total > 0 and int(e.mult.max()) == (2 if name == "nonbinary" else 1)
    assert abs(e.loss_rel - l_rel) < 1e-12 * max(1.0, abs(l_rel))
    assert np.abs(e.grad - g_rel).max() < 1e-12
    assert np.array_equal(g_rel != 0, e.mult > 0)
    if k_neg == 0 or k_nm == 0:
        assert all(info[0 if k_neg == 0 else 1] == (0, 0, 0) for info in e.info)


def test_nonbinary_targets_enter_the_mean_twice():
    c = LR.nonbinary_case()
    e = LR.relation_expectation(c, 2, 3, "key")
    tq = LR.target_rows(c)
    q_of = {int(r): q for q, r in enumerate(tq)}
    assert e.mult[0, q_of[3], q_of[1], 2] == 2 and e.mult[0, q_of[0], q_of[5], 4] == 2     # true AND sampled
    assert e.mult[0, q_of[2], q_of[2], 1] == 1                                             # true, not sampled
    assert sorted(np.unique(c["dense"][0].numpy()).tolist()) == [0.0, 0.5, 1.0, 2.0]


def test_key_order():
    x = np.array([-np.inf, -1.0, -2.0 ** -140, -0.0, 0.0, 2.0 ** -149, 2.0 ** -140, 1.0, 1.25, np.inf], dtype=np.float32)
    k = LR.key_of(x).astype(np.int64)
    assert (np.diff(k) > 0).all()                                    # strictly increasing, the two zeros included
    assert k[4] - k[3] == 1 and LR.key_of(np.float32(0.0)) == 0x80000000 and LR.key_of(np.float32(-0.0)) == 0x7FFFFFFF
    z = np.array([[-0.0, 0.0, -0.0, 0.0]], dtype=np.float32)
    cand = np.ones_like(z, dtype=bool)
    assert LR.topk_lowest_index_first(z, cand, 2, "value").tolist() == [[True, True, False, False]]
    assert LR.topk_lowest_index_first(z, cand, 2, "key").tolist() == [[False, True, False, True]]
    assert LR.topk_lowest_index_first(z, cand, 3, "key").tolist() == [[True, True, False, True]]


# --------------------------------------------------------------------------------------------------- preconditions B1-B3
def _one_true_relation(c):
    for b in range(c["B"]):
        pi, ti = c["indices"][b]
        block = c["dense"][b][ti][:, ti]
        assert int((block != 0).sum()) == 1
        assert len(set(pi.tolist())) == len(pi)


def _tied_steps_of_row(e, c, b, prob, row):
    flat = np.nonzero(e.images[b].tied[prob].reshape(-1))[0]
    return {LR.position(f, c["N"], c["R"])[1] for f in flat if LR.position(f, c["N"], c["R"])[0] == row}


@pytest.mark.parametrize("which", ["mid", "last"])
def test_steps_case_preconditions(which):
    c = LR.steps_case()
    N, R = c["N"], c["R"]
    assert (N, R, c["B"]) == (24, 50, 1) and N * R == 4 * LR.STEP + 176
    _one_true_relation(c)
    assert set(np.unique(c["pred_rel"].numpy()).tolist()) == {-0.5, 0.0, 0.5}
    k_neg, k_nm = c["ks"][which]
    e = LR.relation_expectation(c, k_neg, k_nm, "key")
    for prob, (k, tied, need) in enumerate(e.info[0]):
        assert k == (k_neg, k_nm)[prob] and 0 < need < tied, e.info
        row, step, wave = e.cuts[0][prob]
        assert step >= 1 and wave >= 1, e.cuts
        assert len(_tied_steps_of_row(e, c, 0, prob, row)) >= 3
        if which == "last":
            assert step == 4                                        # the partial step: 176 live lanes
    if which == "mid":
        assert [cut[1] for cut in e.cuts[0]] == [2, 1]


def test_rows_case_preconditions():
    c = LR.rows_case()
    assert (c["N"], c["R"], c["B"]) == (264, 3, 1)
    _one_true_relation(c)
    assert int((c["indices"][0][0] >= 256).sum()) >= 2 and int((c["indices"][0][0] < 256).sum()) >= 2
    k_neg, k_nm = c["ks"]["rows"]
    e = LR.relation_expectation(c, k_neg, k_nm, "key")
    for prob, (k, tied, need) in enumerate(e.info[0]):
        assert 0 < need < tied
        row, step, wave = e.cuts[0][prob]
        assert row >= 256 and step >= 1, e.cuts
        # tied candidates in rows 0..255 AND in rows 256..row-1: both trips of the prefix loop carry a count
        rows = np.nonzero(e.images[0].tied[prob].reshape(c["N"], -1).any(1))[0]
        assert (rows < 256).any() and ((rows >= 256) & (rows < row)).any()


def test_scan_case_preconditions():
    c = LR.scan_case()
    N, T = c["N"], LR.SCAN_T
    assert (N, c["R"], c["B"]) == (1030, 1, 1) and len(c["indices"][0][0]) == T
    _one_true_relation(c)
    pi = c["indices"][0][0].numpy()
    un = np.setdiff1d(np.arange(N), pi)
    assert (pi >= 1024).any() and (un < 1024).any() and (un >= 1024).any()
    tq = LR.target_rows(c)
    q_of = {int(r): q for q, r in enumerate(tq)}
    deep = 0
    for a, o, _ in c["extra"]:
        assert a >= T or o >= T                                     # a row / column of an UNMATCHED query
        assert c["dense"][0][a, o, 0] == 1
        deep += int(max(q_of[a], q_of[o]) >= 1024 and max(a, o) >= 1024)
    assert deep >= 3                                                # ... whose query lies in the scan's second chunk
    k_neg, k_nm = c["ks"]["scan"]
    e = LR.relation_expectation(c, k_neg, k_nm, "key")
    for prob, (k, tied, need) in enumerate(e.info[0]):
        assert 0 < need < tied
    assert e.cuts[0][1][0] >= 1024
    # every sampled candidate AT the threshold has target 0 (the ticket route's loss does not depend on the choice); the
    # target-1 elements outside the block lie strictly above (sampled) or below (not sampled) it
    s = e.images[0]
    assert not (s.t[s.tied[0] | s.tied[1]] != 0).any()
    outside_true = (s.t != 0) & s.cand[1]
    assert int(outside_true.sum()) == len(c["extra"])
    assert int((outside_true & s.sel[1]).sum()) == len(c["extra"]) - 1 and int((outside_true & ~s.sel[1]).sum()) == 1
    # the connectivity target of the oracle sees them
    assert int((s.t != 0).any(-1).sum()) == len(c["extra"]) + 1


# ------------------------------------------------------------------------------------------------------ preconditions B4
@pytest.mark.parametrize("family", LR.RADIX_FAMILIES)
def test_radix_family_preconditions(family):
    c = LR.radix_case(family)
    assert (c["N"], c["R"], c["B"]) == (16, 8, 1) and len(c["indices"][0][0]) == 6
    _one_true_relation(c)
    x = c["pred_rel"].numpy().reshape(-1)
    key = LR.key_of(x)
    assert np.isfinite(x).all()
    if family == "one_bin":
        assert (x >= 1).all() and (x < 1.25).all() and len(np.unique(key >> 21)) == 1 and len(np.unique(x)) == x.size
    elif family == "one_bin_negative":
        assert (x <= -1).all() and (x > -1.25).all() and len(np.unique(key >> 21)) == 1 and len(np.unique(x)) == x.size
        assert (key < 0x80000000).all()                             # complemented keys
    elif family in ("low_bits", "low_bits_negative"):
        assert len(np.unique(key >> 10)) == 1 and len(np.unique(key)) < x.size      # 22 shared bits, duplicates
        assert (x > 0).all() if family == "low_bits" else (x < 0).all()
    elif family == "powers":
        assert len(np.unique(key >> 21)) > 100 and (x > 0).any() and (x < 0).any()
        assert np.abs(x).min() < 2.0 ** -90 and np.abs(x).max() > 16
    else:
        assert len(np.unique(key)) == 6
        hit = False
        for k in LR.RADIX_KS:
            e = LR.relation_expectation(c, k, k, "key")
            s = e.images[0]
            for prob in range(2):
                cand = s.cand[prob].reshape(-1)
                both = (key[cand] == 0x80000000).any() and (key[cand] == 0x7FFFFFFF).any()
                thr = key[s.tied[prob].reshape(-1)]
                hit |= bool(both and len(thr) and thr[0] in (0x80000000, 0x7FFFFFFF) and 0 < e.info[0][prob][2] < e.info[0][prob][1])
        assert hit                                                  # a threshold at a zero, cut among tied zeros
    # the sweep takes one element, a few, and every candidate
    n_false, n_nm = 6 * 6 * 8 - 1, (16 * 16 - 36) * 8
    ks = [LR.relation_expectation(c, k, k, "key").info[0] for k in LR.RADIX_KS]
    assert [(a[0], b[0]) for a, b in ks] == [(1, 1), (2, 2), (37, 37), (n_false, 500), (n_false, n_nm)]


# ------------------------------------------------------------------------------------------------------ preconditions B5
def test_degenerate_case_preconditions():
    c = LR.degenerate_case()
    assert (c["B"], c["N"], c["R"]) == (4, 9, 7)
    assert [len(a) for a, _ in c["indices"]] == [9, 0, 3, 5]
    assert [len(t) for t in c["trips"]] == [3, 0, 0, 2]
    e = LR.relation_expectation(c, 2, 2, "key")
    assert e.info[0][1] == (0, 0, 0) and e.info[0][0][0] == 6      # nothing outside the block of image 0
    assert e.info[1] == [(0, 0, 0)] * 2 and e.info[2] == [(0, 0, 0)] * 2
    assert not e.mult[1].any() and not e.mult[2].any()
    assert all(0 < need < tied for _, tied, need in e.info[3])      # image 3: ties at both cuts


def test_case_generators_are_cached_and_deterministic():
    assert LR.steps_case() is LR.steps_case()
    LR.steps_case.cache_clear()
    a = LR.rows_case()
    LR.rows_case.cache_clear()
    b = LR.rows_case()
    assert torch.equal(a["pred_rel"], b["pred_rel"]) and a["ks"] == b["ks"]
