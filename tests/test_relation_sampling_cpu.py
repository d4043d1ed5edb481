"""CPU: the relation loss's sampling policies (largest | random | all per candidate class) -- the random key's
known answers and distinctness, the twin (tests/relation_sampling_restated.py) anchored to the existing restatements and to the
reference's own composition, the uniformity of the keyed selection, the policy entries' argument checks and the sampler state.
No GPU: the kernels themselves are tests/test_gpu_relation_sampling.py."""
import ctypes
import itertools
import random

import numpy as np
import pytest
import torch

import loss_restated as LR
import relation_loss_all_restated as RA
import relation_sampling_restated as RS


# ------------------------------------------------------------------------------------------------------------------- the key
def test_philox_known_answers():
    """Philox4x32-10: the zero vector and the pi-digits vector of the Random123 known-answer set."""
    assert RS.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert RS.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == (
        0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_class_keys_read_seed_and_stream_as_64_bit_words():
    assert RS.class_keys(2 ** 63 + 5, 2 ** 32 + 7, 3, 1) == RS.philox4x32_10((3, 1, 7, 1), (5, 2 ** 31))[:2]
    assert RS.class_keys(-1, 0, 0, 0) == RS.class_keys(2 ** 64 - 1, 0, 0, 0)       # modulo 2^64
    assert RS.class_keys(0, 0, 0, 0) != RS.class_keys(0, 0, 0, 1) != RS.class_keys(0, 1, 0, 1)


@pytest.mark.parametrize("seed,stream,b,prob", [(0, 0, 0, 0), (1234, 7, 3, 1), (2 ** 63 + 5, 2 ** 40, 255, 1)])
def test_keys_are_distinct(seed, stream, b, prob):
    """Every step of the key is a bijection of 32 bits: no two flat indices below 2^22 share a key."""
    keys = RS.sample_key(np.arange(1 << 22, dtype=np.uint32), *RS.class_keys(seed, stream, b, prob))
    assert keys.dtype == np.uint32 and np.unique(keys).size == 1 << 22


# ------------------------------------------------------------------------------------------------------------------- anchors
@pytest.mark.parametrize("case", ["plain", "degenerate", "nonbinary"])
@pytest.mark.parametrize("k_neg,k_nm", [(2, 3), (80, 80), (0, 3), (3, 0)])
def test_twin_with_both_largest_is_the_existing_restatement(case, k_neg, k_nm):
    c = {"plain": LR.plain_case, "degenerate": LR.degenerate_case, "nonbinary": LR.nonbinary_case}[case]()
    want = LR.relation_expectation(c, k_neg, k_nm, "key")
    got = RS.expectation(c, ("largest", k_neg), ("largest", k_nm), seed=9, stream=4)
    assert np.array_equal(got.mult, want.mult) and got.total == want.total
    assert np.array_equal(got.grad, want.grad, equal_nan=True)
    assert got.loss_rel == want.loss_rel or (np.isnan(got.loss_rel) and np.isnan(want.loss_rel))


@pytest.mark.parametrize("case", ["plain", "degenerate"])
def test_twin_with_both_all_is_the_unsampled_restatement(case):
    c = {"plain": LR.plain_case, "degenerate": LR.degenerate_case}[case]()
    got = RS.expectation(c, ("all", None), ("all", None))
    assert int(got.mult.min()) == 1 and int(got.mult.max()) == 1 and got.total == got.mult.size
    l_rel, _, g_rel, _ = RA.restate(c["pred_rel"], c["pred_conn"], c["dense"], c["indices"], c["costs"], nm_cost=LR.NM_COST)
    assert abs(got.loss_rel - l_rel) <= 1e-12 * abs(l_rel)
    assert float(np.abs(got.grad - g_rel).max()) <= 1e-12 * float(np.abs(g_rel).max())


def reference_composition(c, negatives, nonmatching, seed, stream, monkeypatch):
    """loss_rel of the criterion's reference composition (SceneGraphGenerationLoss._loss_relations per image, float64, CPU) with
    ``random.sample`` answering with the ranks, in the reference's candidate lists, of the elements the twin selects."""
    import egtr_amd.egtr as E
    N, R = c["N"], c["R"]
    crit = RA.criterion(N, R, True)
    crit.nonmatching_cost = torch.tensor(LR.NM_COST, dtype=torch.float64)
    crit.rel_sample_negatives, crit.rel_sample_nonmatching = negatives[1], nonmatching[1]
    crit.rel_sample_negatives_largest = negatives[0] != "random"
    crit.rel_sample_nonmatching_largest = nonmatching[0] != "random"
    e = RS.expectation(c, negatives, nonmatching, seed, stream)
    losses, draws = [], []
    for b in range(c["B"]):
        pi, ti = c["indices"][b]
        T = len(pi)
        unmatched = torch.tensor([q for q in range(N) if q not in set(pi.tolist())], dtype=torch.int64)
        full_src = torch.cat([pi, unmatched])
        full_tgt = torch.cat([ti, torch.arange(T, N)])
        cost = torch.cat([c["costs"][b].double(), torch.full((N - T,), LR.NM_COST, dtype=torch.float64)])
        pred = c["pred_rel"][b].double()[full_src][:, full_src]
        tgt = c["dense"][b].double()[full_tgt][:, full_tgt]
        s = e.images[b]
        expected = []   # the draws this image makes, in the reference's order: block candidates, then non-matching
        matched = torch.zeros(N, dtype=torch.bool)
        matched[:T] = True
        lists = ((tgt[:T, :T] != 1.0), ~(matched[:, None] & matched[None, :])[:, :, None].expand(N, N, R))
        for prob, (policy, cand) in enumerate(zip((negatives, nonmatching), lists)):
            if policy[0] != "random" or policy[1] == 0 or s.n_true == 0:
                continue
            sel = torch.as_tensor(s.sel[prob])[full_src][:, full_src]            # the twin's choice, in the permuted order
            sel = sel[:T, :T] if prob == 0 else sel
            assert not bool((sel & ~cand).any())
            expected.append((int(cand.sum()), torch.nonzero(sel[cand]).reshape(-1).tolist()))

        def fake_sample(population, k, expected=expected):
            n, ranks = expected.pop(0)
            assert len(population) == n and k == len(ranks)
            draws.append(k)
            # as an int64 array: the reference wraps the draw in torch.tensor(), and an EMPTY list becomes a float tensor that
            # cannot index (the reference raises on an image whose candidate class is empty -- degenerate_case's image 0 has
            # every query matched, so nothing lies outside the block); an empty int64 array indexes nothing, which is the value
            return np.asarray(ranks, dtype=np.int64)

        monkeypatch.setattr(E.random, "sample", fake_sample)
        losses.append(crit._loss_relations(pred, tgt, cost, crit.rel_sample_negatives, crit.rel_sample_nonmatching))
        assert not expected
    monkeypatch.undo()
    return float(torch.cat(losses).mean()), e, draws


@pytest.mark.parametrize("case", ["plain", "degenerate"])
@pytest.mark.parametrize("negatives,nonmatching", [(("random", 2), ("random", 3)), (("random", 2), ("all", None)),
                                                   (("all", None), ("random", 3))])
def test_twin_equals_the_reference_composition_given_the_same_draws(case, negatives, nonmatching, monkeypatch):
    c = {"plain": LR.plain_case, "degenerate": LR.degenerate_case}[case]()
    state = random.getstate()
    got, e, draws = reference_composition(c, negatives, nonmatching, 77, 3, monkeypatch)
    assert random.getstate() == state and draws          # the patched draws were the only ones
    assert abs(got - e.loss_rel) <= 1e-12 * abs(e.loss_rel), (got, e.loss_rel)


# ---------------------------------------------------------------------------------------------------------------- uniformity
@pytest.mark.parametrize("seed", RS.UNIFORM_SEEDS)
@pytest.mark.parametrize("ks", RS.UNIFORM_KS)
def test_keyed_selection_is_uniform_to_second_order(seed, ks):
    """4096 draws (image 0 .. 255 x stream 0 .. 15) of k out of the 26 block candidates and of the 81 outside elements of the
    uniform case: every candidate's inclusion count within 5 sigma of S k / n, every pair's co-inclusion count within 5 sigma of
    S k (k - 1) / (n (n - 1)) (binomial sigmas).  A condition on the DEFINITION of the key: deterministic, no GPU."""
    S = RS.UNIFORM_B * RS.UNIFORM_STREAMS
    worst = []
    for prob, (flat, k) in enumerate(zip(RS.uniform_candidates(), ks)):
        n = len(flat)
        assert n == (26, 81)[prob] and 0 < k < n
        inc = np.zeros((S, n), dtype=np.int64)
        for i, (b, stream) in enumerate(itertools.product(range(RS.UNIFORM_B), range(RS.UNIFORM_STREAMS))):
            keys = RS.sample_key(flat, *RS.class_keys(seed, stream, b, prob))
            inc[i, np.argsort(keys)[::-1][:k]] = 1
        assert (inc.sum(1) == k).all()
        p1, p2 = k / n, k * (k - 1) / (n * (n - 1))
        s1, s2 = np.sqrt(S * p1 * (1 - p1)), np.sqrt(S * p2 * (1 - p2))
        d1 = np.abs(inc.sum(0) - S * p1)
        pair = inc.T @ inc
        d2 = np.abs(pair[np.triu_indices(n, 1)] - S * p2)
        worst.append((float(d1.max() / s1), float(d2.max() / s2) if s2 > 0 else 0.0))
        assert (d1 <= 5 * s1).all(), (prob, k, float(d1.max() / s1))
        assert (d2 <= 5 * s2).all(), (prob, k, float(d2.max()), s2)
    print(f"seed {seed} k {ks}: worst (inclusion, pair) in sigmas per class {worst}")


# ------------------------------------------------------------------------------------------------------- entries without a GPU
E_ARG, E_UNSUPPORTED = -1, -3
TARGET_FORMATS = (0, 1, 2)     # EGTR_REL_TARGET_DENSE / _WORDS / _WIDE


def _plausible():
    raw = ctypes.create_string_buffer(4096 + 16)
    return raw, (ctypes.addressof(raw) + 15) & ~15


@pytest.mark.parametrize("deterministic", [0, 1])
@pytest.mark.parametrize("target_format", TARGET_FORMATS)
def test_policy_entries_reject_bad_arguments_before_any_hip_call(target_format, deterministic):
    from egtr_amd import _lib
    fn = _lib.lib().egtr_relation_loss_f32
    keep, p = _plausible()

    def call(ptrs=None, N=4, R=3, neg=0, nm=0, pol=(1, 2), B=1, fmt=target_format, ws=p):
        a = [p] * 8 if ptrs is None else ptrs
        return fn(None, a[0], a[1], a[2], fmt, a[3], a[4], a[5], a[6], B, N, R, 1.0, neg, nm, a[7], p, p, ws, pol[0], pol[1], 5,
                  0, deterministic)

    for missing in range(8):     # pred_rel, pred_conn, target, pred_idx, tgt_idx, match_cost, out_offsets, loss_out
        assert call([None if i == missing else p for i in range(8)]) == E_ARG, missing
    assert call(ws=None) == E_ARG                                                                        # workspace
    for pol in ((3, 0), (0, 3), (-1, 1), (2, 7)):
        assert call(pol=pol) == E_ARG, pol
    for bad in (-1, 3):                                                  # an unknown target format, all else valid
        assert call(fmt=bad) == E_ARG and call(fmt=bad, pol=(0, 0)) == E_ARG, bad
    assert call(neg=-1) == E_ARG and call(B=0) == E_ARG
    # the flat index of a random class is 32 bits; the selected count of a whole class a 32-bit int
    limit = {0: None, 1: 65, 2: 257}[target_format]
    if limit is not None:
        assert call(R=limit) == E_UNSUPPORTED and call(R=limit, pol=(0, 0)) == E_UNSUPPORTED
        assert call(R=limit, pol=(0, 5)) == E_ARG           # the policy check comes first
    if target_format != 1:                                   # (256 predicates: not in one word)
        assert call(N=4096, R=256, pol=(1, 0)) == E_UNSUPPORTED      # N N R = 2^32 with a random class
        assert call(N=4096, R=256, pol=(0, 2)) == E_UNSUPPORTED      # ... and >= 2^31 with a whole one
    if target_format == 0:
        assert call(N=4096, R=1024) == E_UNSUPPORTED                  # the limit N R < 2^22
    del keep


def test_launch_binding_rejects_bad_policies_and_counts():
    from egtr_amd.kernels import heads
    x = torch.zeros(1, 2, 2, 3)
    with pytest.raises(ValueError, match="policy"):
        heads.relation_loss_policy_launch(x, x, x, False, x, x, x, x, 1.0, ("smallest", 1), ("all", None))
    with pytest.raises(ValueError, match="count"):
        heads.relation_loss_policy_launch(x, x, x, False, x, x, x, x, 1.0, ("random", None), ("all", None))
    assert heads.RELATION_POLICIES == {"largest": 0, "random": 1, "all": 2}


# -------------------------------------------------------------------------------------------------------------- sampler state
def test_sampler_state():
    from egtr_amd import ops
    assert ops.relation_sampler() == "python"                      # the default: the reference's draws
    seed0, stream0 = ops.relation_sampler_state()
    try:
        assert ops.set_relation_sampler("device", seed=11) == "python"
        assert ops.relation_sampler() == "device" and ops.relation_sampler_state() == (11, 0)
        assert ops._next_relation_stream() == (11, 0) and ops.relation_sampler_state() == (11, 1)
        assert ops.set_relation_sampler("python") == "device"
        assert ops.relation_sampler_state() == (11, 1)             # a name alone keeps seed and stream
        with ops.relation_sampler_mode("device", seed=2 ** 63 + 5):
            assert ops.relation_sampler() == "device" and ops.relation_sampler_state() == (2 ** 63 + 5, 0)
            with ops.relation_sampler_mode("python"):
                assert ops.relation_sampler() == "python"
            assert ops.relation_sampler() == "device"
        assert ops.relation_sampler() == "python"
        with pytest.raises(RuntimeError):
            with ops.relation_sampler_mode("device"):
                raise RuntimeError("x")
        assert ops.relation_sampler() == "python"                  # restored on an exception too
        ops.set_relation_sampler_state(3, 40)
        assert ops.relation_sampler_state() == (3, 40)
        for bad in ("gpu", None, 1):
            with pytest.raises(ValueError):
                ops.set_relation_sampler(bad)
            with pytest.raises(ValueError):
                ops.relation_sampler_mode(bad)
        assert ops.relation_sampler() == "python"
    finally:
        ops.set_relation_sampler("python")
        ops.set_relation_sampler_state(seed0, stream0)


def test_default_seed_is_torchs_initial_seed(monkeypatch):
    from egtr_amd import ops
    monkeypatch.setattr(ops, "_RELATION_SAMPLER_SEED", None)
    monkeypatch.setattr(ops, "_RELATION_SAMPLER_STREAM", 0)
    assert ops.relation_sampler_state() == (int(torch.initial_seed()), 0)


def test_criterion_keeps_a_random_class_on_the_composition_under_the_python_sampler():
    """The route decision alone (no kernel runs): which configurations the policy kernels take."""
    from egtr_amd import ops
    crit = RA.criterion(11, 6, True)

    def policies(neg, nm, neg_largest=True, nm_largest=True):
        crit.rel_sample_negatives, crit.rel_sample_nonmatching = neg, nm
        crit.rel_sample_negatives_largest, crit.rel_sample_nonmatching_largest = neg_largest, nm_largest
        return crit._sampling_policies(3, 11, 6)

    assert policies(None, None) is None                                               # the un-sampled entries
    assert policies(None, 80) == (("all", None), ("largest", 80))
    assert policies(80, None, neg_largest=False) is None                              # "python": random.sample draws
    with ops.relation_sampler_mode("device"):
        assert policies(80, None, neg_largest=False) == (("random", 80), ("all", None))
        assert policies(2, 3, False, False) == (("random", 2), ("random", 3))
        assert policies(2, 3, True, False) == (("largest", 2), ("random", 3))
    crit.model_training = False
    assert policies(None, 80) is None
