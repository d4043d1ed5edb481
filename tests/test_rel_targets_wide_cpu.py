"""CPU: wide packed relation targets -- int64 [B, N, N, W] words with W = ceil(R / 64) for up to 256
predicates: ``pack_relations_wide`` / ``unpack_relations`` against a dense tensor built by hand, the W = 1 form against
``pack_relations``, the argument checks of the four C entries (no GPU: host addresses that no kernel ever sees) and the
criterion on CPU tensors at 100 predicates."""
import ctypes
import os
import re

import pytest
import torch

N = 5
RS = (1, 63, 64, 65, 100, 127, 128, 129, 191, 192, 193, 255, 256)
NEW_ENTRIES = ("egtr_pack_relations_wide_u64", "egtr_relation_loss_wide_bits_f32", "egtr_relation_loss_det_wide_bits_f32",
               "egtr_relation_loss_all_wide_bits_f32")
E_ARG, E_UNSUPPORTED = -1, -3


def triplets(R):
    """image 0: predicates 63 and 64 on ONE pair (as far as R has them), predicate R - 1, a duplicate; image 1: no triplet;
    image 2: every word of one pair"""
    rows = [[1, 2, min(63, R - 1)], [1, 2, min(64, R - 1)], [3, 0, R - 1], [4, 4, 0], [3, 0, R - 1], [0, 0, R // 2]]
    every = [[2, 3, p] for p in range(0, R, 64)] + [[2, 3, R - 1]]
    return [torch.tensor(rows), torch.zeros(0, 3, dtype=torch.int64), torch.tensor(every)]


def dense_by_hand(t, R):
    rel = torch.zeros(N, N, R)
    for s, o, p in t.tolist():
        rel[s, o, p] = 1.0
    return rel


def bit_by_hand(words, b, s, o, p):
    return (int(words[b, s, o, p >> 6]) >> (p & 63)) & 1


@pytest.mark.parametrize("R", RS)
def test_pack_wide_against_dense_by_hand_and_round_trip(R):
    from egtr_amd import targets as T
    trips = triplets(R)
    tg = [{"rel_triplets": t} for t in trips]
    W = (R + 63) // 64
    words = T.pack_relations_wide(tg, N, R, "cpu")
    assert words.dtype == torch.int64 and tuple(words.shape) == (len(trips), N, N, W) and words.is_contiguous()
    for b, t in enumerate(trips):
        dense = dense_by_hand(t, R)
        for s in range(N):                     # every bit of every word, positions >= R included
            for o in range(N):
                for p in range(64 * W):
                    assert bit_by_hand(words, b, s, o, p) == (int(dense[s, o, p]) if p < R else 0), (b, s, o, p)
        back = T.unpack_relations(words, b, R)
        assert back.dtype == torch.float32 and tuple(back.shape) == (N, N, R) and torch.equal(back, dense)
    assert int((words[1] != 0).sum()) == 0
    assert bit_by_hand(words, 0, 3, 0, R - 1) == 1
    if R > 64:
        assert bit_by_hand(words, 0, 1, 2, 63) == 1 and bit_by_hand(words, 0, 1, 2, 64) == 1
        assert int(words[0, 1, 2, 0]) < 0 and int(words[0, 1, 2, 1]) & 1 == 1         # bit 63 of word 0, bit 0 of word 1
    dense_tg = T.dense_targets(tg, N, R, "cpu", rel_bits=words)                         # wide words as ``rel_bits``
    for b, t in enumerate(trips):
        assert torch.equal(dense_tg[b]["rel"], dense_by_hand(t, R)) and dense_tg[b]["rel_triplets"] is t


@pytest.mark.parametrize("R", [r for r in RS if r <= 64])
def test_one_word_per_pair_is_the_narrow_form(R):
    from egtr_amd import targets as T
    tg = [{"rel_triplets": t} for t in triplets(R)]
    assert torch.equal(T.pack_relations_wide(tg, N, R, "cpu"), T.pack_relations(tg, N, R, "cpu")[..., None])


def test_value_errors():
    from egtr_amd import targets as T
    assert T.MAX_PACKED_REL_LABELS == 256 and T.MAX_REL_LABELS == 64
    good = [{"rel_triplets": torch.tensor([[0, 1, 2]])}]
    for R in (0, 257, -3):
        with pytest.raises(ValueError):
            T.pack_relations_wide(good, N, R, "cpu")
    for row in ([0, 1, 100], [N, 0, 3], [0, N, 3], [-1, 0, 3], [0, 0, -1], [0, 0, 2 ** 40]):
        with pytest.raises(ValueError, match="outside"):
            T.pack_relations_wide([good[0], {"rel_triplets": torch.tensor([row])}], N, 100, "cpu")
    with pytest.raises(ValueError):
        T.unpack_relations(torch.zeros(1, N, N, 3, dtype=torch.int64), 0, 100)         # 100 predicates are two words
    with pytest.raises(ValueError, match="at most 64"):                                 # the narrow form is what it was
        T.pack_relations(good, N, 65, "cpu")


def test_new_symbols_are_bound_and_declared():
    from egtr_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "egtr_hip.h")) as f:
        header = f.read()
    h = _lib.lib()
    for name in NEW_ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(h, name)
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    sib = {"egtr_pack_relations_wide_u64": "egtr_pack_relations_u64", "egtr_relation_loss_wide_bits_f32": "egtr_relation_loss_bits_f32",
           "egtr_relation_loss_det_wide_bits_f32": "egtr_relation_loss_det_bits_f32",
           "egtr_relation_loss_all_wide_bits_f32": "egtr_relation_loss_all_bits_f32"}
    for name, other in sib.items():
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[other]                          # the siblings' argument lists
    assert h.egtr_abi_version() == 6 and _lib.ABI_VERSION == 6


def test_c_entries_validate_without_a_gpu():
    """NULL operands are EGTR_E_ARG, num_rel = 257 is EGTR_E_UNSUPPORTED, both before any HIP call; the narrow entries still
    answer EGTR_E_UNSUPPORTED at 65."""
    from egtr_amd import _lib
    h = _lib.lib()
    raw = ctypes.create_string_buffer(64 + 16)
    p = (ctypes.addressof(raw) + 15) & ~15
    pack = h.egtr_pack_relations_wide_u64
    assert pack(None, None, None, 2, 3, 7, 100, None) == E_ARG
    for ptrs in ((None, p, p), (p, None, p), (p, p, None)):
        assert pack(None, ptrs[0], ptrs[1], 2, 3, 7, 100, ptrs[2]) == E_ARG
    assert pack(None, p, p, 2, 3, 7, 257, p) == E_UNSUPPORTED
    for sizes in ((0, 3, 7, 100), (2, -1, 7, 100), (2, 3, 0, 100), (2, 3, 7, 0)):
        assert pack(None, p, p, *sizes, p) == E_ARG, sizes
    assert h.egtr_pack_relations_u64(None, p, p, 2, 3, 7, 65, p) == E_UNSUPPORTED
    for name in ("egtr_relation_loss_wide_bits_f32", "egtr_relation_loss_det_wide_bits_f32"):
        entry = getattr(h, name)

        def call(ptrs=(p,) * 7, sizes=(2, 7, 100), out=(p, p, p, p), entry=entry):
            return entry(None, *ptrs, *sizes, 1.0, 80, 80, *out)
        assert call(ptrs=(None,) * 7, out=(None,) * 4) == E_ARG
        for i in range(7):
            assert call(ptrs=tuple(None if j == i else p for j in range(7))) == E_ARG, (name, i)
        for i in range(4):
            assert call(out=tuple(None if j == i else p for j in range(4))) == E_ARG, (name, i)
        assert call(sizes=(2, 7, 257)) == E_UNSUPPORTED
        assert call(sizes=(2, 7, 0)) == E_ARG and call(sizes=(0, 7, 100)) == E_ARG
        assert call(sizes=(1, 4097, 100)) == E_UNSUPPORTED                   # the dense entries' limit on N
    entry = h.egtr_relation_loss_all_wide_bits_f32

    def call_all(ptrs=(p,) * 7, sizes=(2, 7, 100), out=(p, p, p, p)):
        return entry(None, *ptrs, *sizes, 1.0, *out)
    assert call_all(ptrs=(None,) * 7, out=(None,) * 4) == E_ARG
    for i in range(7):
        assert call_all(ptrs=tuple(None if j == i else p for j in range(7))) == E_ARG, i
    assert call_all(out=(None, p, p, p)) == E_ARG and call_all(out=(p, p, p, None)) == E_ARG
    assert call_all(out=(p, None, p, p)) == E_ARG and call_all(out=(p, p, None, p)) == E_ARG          # ONE NULL gradient
    assert call_all(sizes=(2, 7, 257)) == E_UNSUPPORTED
    assert call_all(sizes=(2, 7, 257), out=(p, None, None, p)) == E_UNSUPPORTED                        # value-only form
    assert h.egtr_relation_loss_bits_f32(None, *(p,) * 7, 2, 7, 65, 1.0, 80, 80, p, p, p, p) == E_UNSUPPORTED
    assert h.egtr_relation_loss_det_bits_f32(None, *(p,) * 7, 2, 7, 65, 1.0, 80, 80, p, p, p, p) == E_UNSUPPORTED
    assert h.egtr_relation_loss_all_bits_f32(None, *(p,) * 7, 2, 7, 65, 1.0, p, p, p, p) == E_UNSUPPORTED


def test_launch_helpers_select_the_entry_by_the_rank_of_the_words(monkeypatch):
    """4-D words take the wide entries, 3-D words the narrow ones; W != ceil(R / 64) is a RuntimeError (no GPU: the launch is
    recorded, not made)."""
    from egtr_amd import _lib
    from egtr_amd.kernels import heads
    called = []
    monkeypatch.setattr(_lib, "launch", lambda name, *a, **k: called.append(name))
    monkeypatch.setattr(_lib, "lib", lambda: type("L", (), {"egtr_relation_loss_workspace_bytes": staticmethod(lambda b, n: 16),
                                                            "egtr_relation_loss_det_workspace_bytes": staticmethod(lambda b, n: 16),
                                                            "egtr_relation_loss_all_workspace_bytes": staticmethod(lambda b, n: 16)})())
    monkeypatch.setattr(heads, "_chk", lambda t, *a, **k: t)
    B, R = 2, 100
    pr, pc = torch.zeros(B, N, N, R), torch.zeros(B, N, N, 1)
    z = torch.zeros(1, dtype=torch.int64)
    wide, narrow = torch.zeros(B, N, N, 2, dtype=torch.int64), torch.zeros(B, N, N, dtype=torch.int64)
    heads.relation_loss_launch(pr, pc, wide, True, z, z, z, z, 1.0, 80, 80)
    heads.relation_loss_launch(pr, pc, wide, True, z, z, z, z, 1.0, 80, 80, deterministic=True)
    heads.relation_loss_all_launch(pr, pc, wide, True, z, z, z, z, 1.0)
    heads.relation_loss_launch(pr, pc, narrow, True, z, z, z, z, 1.0, 80, 80)
    heads.relation_loss_all_launch(pr, pc, narrow, True, z, z, z, z, 1.0)
    assert called == ["egtr_relation_loss_wide_bits_f32", "egtr_relation_loss_det_wide_bits_f32",
                      "egtr_relation_loss_all_wide_bits_f32", "egtr_relation_loss_bits_f32", "egtr_relation_loss_all_bits_f32"]
    for bad in (torch.zeros(B, N, N, 1, dtype=torch.int64), torch.zeros(B, N, N, 3, dtype=torch.int64)):
        with pytest.raises(RuntimeError, match="wide rel_bits"):
            heads.relation_loss_launch(pr, pc, bad, True, z, z, z, z, 1.0, 80, 80)
        with pytest.raises(RuntimeError, match="wide rel_bits"):
            heads.relation_loss_all_launch(pr, pc, bad, True, z, z, z, z, 1.0)


@pytest.mark.parametrize("neg,nm,training", [(None, None, True), (80, 80, True), (80, 80, False)])
def test_criterion_on_cpu_tensors_at_100_predicates_equal_for_both_target_forms(neg, nm, training):
    """the whole criterion (``forward`` packs the wide words once) and the terms called on their own"""
    from egtr_amd import targets as T
    from egtr_amd.deformable_detr import DeformableDetrHungarianMatcher
    from egtr_amd.egtr import SceneGraphGenerationLoss
    Nq, R, C, k = 9, 100, 5, 4
    g = torch.Generator().manual_seed(11)
    trip, dense = [], []
    for n in (17, 0, 40):
        t = torch.stack([torch.randint(0, k, (n,), generator=g), torch.randint(0, k, (n,), generator=g),
                         torch.randint(0, R, (n,), generator=g)], 1)
        if n:
            t[0, 2], t[1], t[2] = R - 1, torch.tensor([1, 2, 63]), torch.tensor([1, 2, 64])
            t = torch.cat([t, t[:3]])
        base = {"class_labels": torch.randint(0, C, (k,), generator=g), "boxes": torch.rand(k, 4, generator=g) * 0.5 + 0.25}
        rel = torch.zeros(Nq, Nq, R)
        for s, o, p in t.tolist():
            rel[s, o, p] = 1.0
        trip.append(dict(base, rel_triplets=t))
        dense.append(dict(base, rel=rel))
    matcher = DeformableDetrHungarianMatcher(class_cost=1.0, bbox_cost=5.0, giou_cost=2.0, smoothing=1e-14)
    crit = SceneGraphGenerationLoss(matcher=matcher, num_object_queries=Nq, num_classes=C, num_rel_labels=R, eos_coef=0.1,
                                    losses=["labels", "boxes", "relations", "uncertainty"], smoothing=1e-14,
                                    rel_sample_negatives=neg, rel_sample_nonmatching=nm, model_training=training,
                                    focal_alpha=0.25, rel_sample_negatives_largest=True, rel_sample_nonmatching_largest=True)
    B = len(trip)
    outputs = dict(logits=torch.randn(B, Nq, C, generator=g), pred_boxes=torch.rand(B, Nq, 4, generator=g) * 0.5 + 0.25,
                   pred_rel=torch.randn(B, Nq, Nq, R, generator=g), pred_connectivity=torch.randn(B, Nq, Nq, 1, generator=g))
    packs = []
    orig = T.pack_relations_wide
    T.pack_relations_wide = lambda *a, **kw: (packs.append(1), orig(*a, **kw))[1]
    try:
        la = crit(outputs, trip)
    finally:
        T.pack_relations_wide = orig
    assert len(packs) == 1 and crit._rel_bits_cache is None                  # packed wide, once per step
    lb = crit(outputs, dense)
    assert set(la) == set(lb) and {"loss_rel", "loss_connectivity", "uncertainty"} <= set(la)
    for name in la:
        assert torch.equal(la[name], lb[name]), name
    indices, costs = matcher(outputs, dense)
    for term in (crit.loss_relations, crit.loss_uncertainty):
        a, b = term(outputs, trip, indices, costs, 1.0), term(outputs, dense, indices, costs, 1.0)
        for name in a:
            assert torch.equal(a[name], b[name]), name
    words = crit._rel_bits(trip, torch.device("cpu"))
    assert tuple(words.shape) == (B, Nq, Nq, 2)
