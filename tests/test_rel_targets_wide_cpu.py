"""CPU: wide packed relation targets -- int64 [B, N, N, W] words with W = ceil(R / 64) for up to 256
predicates: ``pack_relations_wide`` / ``unpack_relations`` against a dense tensor built by hand, the W = 1 form against
``pack_relations``, the argument checks of the C entries (no GPU: host addresses that no kernel ever sees) and the
criterion on CPU tensors at 100 predicates."""
import ctypes
import os
import re

import pytest
import torch

N = 5
RS = (1, 63, 64, 65, 100, 127, 128, 129, 191, 192, 193, 255, 256)
LOSS_ENTRIES = ("egtr_relation_loss_workspace_bytes", "egtr_relation_loss_f32", "egtr_relation_loss_all_workspace_bytes",
                "egtr_relation_loss_all_f32")
DENSE, WORDS, WIDE = 0, 1, 2                                                             # EGTR_REL_TARGET_*
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
    for name in ("egtr_pack_relations_wide_u64",) + LOSS_ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(h, name)
        assert re.search(r"\b(int|long long)\s+" + name + r"\s*\(", header), name
    assert _lib.SIGNATURES["egtr_pack_relations_wide_u64"] == _lib.SIGNATURES["egtr_pack_relations_u64"]
    # the per-form, per-tie-rule and per-policy entries are gone: the four above are every relation-loss name there is
    assert {n for n in _lib.SIGNATURES if n.startswith("egtr_relation_loss")} == set(LOSS_ENTRIES)
    assert set(re.findall(r"\b(egtr_relation_loss\w*)\s*\(", header)) == set(LOSS_ENTRIES)
    for code, macro in ((DENSE, "EGTR_REL_TARGET_DENSE"), (WORDS, "EGTR_REL_TARGET_WORDS"), (WIDE, "EGTR_REL_TARGET_WIDE")):
        assert re.search(r"#define\s+" + macro + r"\s+%d\b" % code, header), macro
    assert h.egtr_abi_version() == 7 and _lib.ABI_VERSION == 7


def _host_pointer():
    raw = ctypes.create_string_buffer(64 + 16)
    return raw, (ctypes.addressof(raw) + 15) & ~15


def test_c_entries_validate_without_a_gpu():
    """NULL operands and an unknown target format are EGTR_E_ARG, num_rel above the format's limit (65 on words, 257 on wide
    words) is EGTR_E_UNSUPPORTED, both before any HIP call: the packing entries, the sampled entry under each target format and
    tie rule, the un-sampled entry under each target format."""
    from egtr_amd import _lib
    h = _lib.lib()
    raw, p = _host_pointer()
    pack = h.egtr_pack_relations_wide_u64
    assert pack(None, None, None, 2, 3, 7, 100, None) == E_ARG
    for ptrs in ((None, p, p), (p, None, p), (p, p, None)):
        assert pack(None, ptrs[0], ptrs[1], 2, 3, 7, 100, ptrs[2]) == E_ARG
    assert pack(None, p, p, 2, 3, 7, 257, p) == E_UNSUPPORTED
    for sizes in ((0, 3, 7, 100), (2, -1, 7, 100), (2, 3, 0, 100), (2, 3, 7, 0)):
        assert pack(None, p, p, *sizes, p) == E_ARG, sizes
    assert h.egtr_pack_relations_u64(None, p, p, 2, 3, 7, 65, p) == E_UNSUPPORTED
    for fmt in (DENSE, WORDS, WIDE):
        for deterministic in (0, 1):
            _sampled_entry_validates(h.egtr_relation_loss_f32, p, fmt, deterministic)
        _all_entry_validates(h.egtr_relation_loss_all_f32, p, fmt)


def _sampled_entry_validates(entry, p, fmt, deterministic):
    R = 100 if fmt == WIDE else 50

    def call(ptrs=(p,) * 7, sizes=(2, 7, R), out=(p, p, p, p), fmt=fmt):
        return entry(None, *ptrs[:3], fmt, *ptrs[3:], *sizes, 1.0, 80, 80, *out, 0, 0, 0, 0, deterministic)
    assert call(ptrs=(None,) * 7, out=(None,) * 4) == E_ARG
    for i in range(7):
        assert call(ptrs=tuple(None if j == i else p for j in range(7))) == E_ARG, i
    for i in range(4):
        assert call(out=tuple(None if j == i else p for j in range(4))) == E_ARG, i
    for bad in (-1, 3):                                                      # all other operands valid
        assert call(fmt=bad) == E_ARG, bad
    if fmt != DENSE:                                                         # (a valid call is never made: these are host addresses)
        assert call(sizes=(2, 7, 65 if fmt == WORDS else 257)) == E_UNSUPPORTED
    assert call(ptrs=(p, p, None, p, p, p, p), sizes=(2, 7, 257)) == E_ARG   # a NULL target comes before the limit
    assert call(sizes=(2, 7, 0)) == E_ARG and call(sizes=(0, 7, R)) == E_ARG
    assert call(sizes=(1, 4097, R)) == E_UNSUPPORTED                         # the limit on N, the same under every format


def _all_entry_validates(entry, p, fmt):
    R = 100 if fmt == WIDE else 50

    def call_all(ptrs=(p,) * 7, sizes=(2, 7, R), out=(p, p, p, p), fmt=fmt):
        return entry(None, *ptrs[:3], fmt, *ptrs[3:], *sizes, 1.0, *out)
    assert call_all(ptrs=(None,) * 7, out=(None,) * 4) == E_ARG
    for i in range(7):
        assert call_all(ptrs=tuple(None if j == i else p for j in range(7))) == E_ARG, i
    assert call_all(out=(None, p, p, p)) == E_ARG and call_all(out=(p, p, p, None)) == E_ARG
    assert call_all(out=(p, None, p, p)) == E_ARG and call_all(out=(p, p, None, p)) == E_ARG          # ONE NULL gradient
    for bad in (-1, 3):
        assert call_all(fmt=bad) == E_ARG, bad
        assert call_all(fmt=bad, out=(p, None, None, p)) == E_ARG
    if fmt != DENSE:
        over = 65 if fmt == WORDS else 257
        assert call_all(sizes=(2, 7, over)) == E_UNSUPPORTED
        assert call_all(sizes=(2, 7, over), out=(p, None, None, p)) == E_UNSUPPORTED                   # value-only form


class _Recorder:
    """stands in for ``_lib.launch``: (name, target_format, policy_neg, policy_nm, deterministic) of every call, picked out
    of the argument tuple by position (None where the un-sampled entry has no such argument)"""

    def __init__(self):
        self.calls = []

    def __call__(self, name, *a, **k):
        if name == "egtr_relation_loss_f32":
            assert len(a) == 23
            self.calls.append((name, a[3], a[18], a[19], a[22]))
        else:
            assert name == "egtr_relation_loss_all_f32" and len(a) == 16
            self.calls.append((name, a[3], None, None, None))


def _fake_library(monkeypatch):
    from egtr_amd import _lib
    rec = _Recorder()
    monkeypatch.setattr(_lib, "launch", rec)
    monkeypatch.setattr(_lib, "lib", lambda: type("L", (), {"egtr_relation_loss_workspace_bytes": staticmethod(lambda b, n: 16),
                                                            "egtr_relation_loss_all_workspace_bytes": staticmethod(lambda b, n: 16)})())
    return rec


def test_launch_helpers_select_the_entry_by_the_rank_of_the_words(monkeypatch):
    """4-D words are target format 2, 3-D words 1, a pointer table 0; ``deterministic`` arrives as 1; integer counts are the
    policies (0, 0); W != ceil(R / 64) is a RuntimeError (no GPU: the launch is recorded, not made)."""
    from egtr_amd.kernels import heads
    rec = _fake_library(monkeypatch)
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
    heads.relation_loss_launch(pr, pc, z, False, z, z, z, z, 1.0, 80, 80, deterministic=True)
    heads.relation_loss_all_launch(pr, pc, z, False, z, z, z, z, 1.0)
    heads.relation_loss_policy_launch(pr, pc, narrow, True, z, z, z, z, 1.0, ("random", 80), ("all", None))
    S, A = "egtr_relation_loss_f32", "egtr_relation_loss_all_f32"
    assert rec.calls == [(S, WIDE, 0, 0, 0), (S, WIDE, 0, 0, 1), (A, WIDE, None, None, None), (S, WORDS, 0, 0, 0),
                         (A, WORDS, None, None, None), (S, DENSE, 0, 0, 1), (A, DENSE, None, None, None), (S, WORDS, 1, 2, 0)]
    for bad in (torch.zeros(B, N, N, 1, dtype=torch.int64), torch.zeros(B, N, N, 3, dtype=torch.int64)):
        with pytest.raises(RuntimeError, match="wide rel_bits"):
            heads.relation_loss_launch(pr, pc, bad, True, z, z, z, z, 1.0, 80, 80)
        with pytest.raises(RuntimeError, match="wide rel_bits"):
            heads.relation_loss_all_launch(pr, pc, bad, True, z, z, z, z, 1.0)


def test_relation_losses_passes_the_deterministic_mode_as_the_flag(monkeypatch):
    """``ops.relation_losses`` on CPU tensors, the launch recorded: inside ``ops.deterministic()`` the entry's flag is 1, outside
    it is 0 (the route table of tests/test_gpu_routes.py names the entry, which is the same under both rules); the sampler
    state is not touched."""
    from egtr_amd import ops
    from egtr_amd.kernels import heads
    rec = _fake_library(monkeypatch)
    monkeypatch.setattr(heads, "_chk", lambda t, *a, **k: t)
    monkeypatch.setattr(ops, "_chk", lambda t, *a, **k: t)
    B, R = 2, 7
    pr, pc = torch.zeros(B, N, N, R), torch.zeros(B, N, N, 1)
    targets = [{"rel": torch.zeros(N, N, R)} for _ in range(B)]
    indices = [(torch.tensor([0, 2]), torch.tensor([1, 0]))] * B
    costs = [torch.zeros(2)] * B
    before = ops.relation_sampler_state()
    prev = ops.set_deterministic(False)
    try:
        ops.relation_losses(pr, pc, targets, indices, costs, 1.0, 80, 80)
        with ops.deterministic():
            ops.relation_losses(pr, pc, targets, indices, costs, 1.0, 80, 80)
        ops.relation_losses(pr, pc, targets, indices, costs, 1.0, 80, 80)
    finally:
        ops.set_deterministic(prev)
    S = "egtr_relation_loss_f32"
    assert rec.calls == [(S, DENSE, 0, 0, 0), (S, DENSE, 0, 0, 1), (S, DENSE, 0, 0, 0)]
    assert ops.relation_sampler_state() == before


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
