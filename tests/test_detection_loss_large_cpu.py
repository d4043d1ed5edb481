"""CPU: the large detection-loss entry (egtr_detection_loss_large_f32) as far as it can be checked without a GPU -- the symbol
and its workspace query, the argument checks that come before any HIP call, the binding's constants against the kernel's, and
that CPU tensors keep the tensor composition in both criteria whatever the route predicate says."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "egtr_detection_loss_large_f32"
QUERY = "egtr_detection_loss_large_workspace_bytes"


def test_entry_is_declared_exported_and_bound():
    from egtr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "egtr_hip.h")).read()
    h = _lib.lib()
    for name in (ENTRY, QUERY):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.SIGNATURES and hasattr(h, name)
    assert _lib.SIGNATURES[ENTRY] == _lib.SIGNATURES["egtr_detection_loss_f32"] + [ctypes.c_void_p]
    assert _lib._RESTYPES[QUERY] is ctypes.c_longlong
    assert h.egtr_abi_version() == 7


def test_constants_of_the_binding_are_the_kernels():
    from egtr_amd import ops
    src = open(os.path.join(ROOT, "egtr_amd", "csrc", "loss.hip")).read()
    assert int(re.search(r"kDetLargeRows = (\d+);", src).group(1)) == ops.DETECTION_LOSS_LARGE_ROWS
    assert int(re.search(r"kDetLargeMaxN = (\d+);", src).group(1)) == ops.DETECTION_LOSS_LARGE_MAX_QUERIES
    assert ops.DETECTION_LOSS_LARGE_MAX_QUERIES == ops.HUNGARIAN_LARGE_MAX_QUERIES
    assert ops.detection_loss_large_route(1) and ops.detection_loss_large_route(65536)
    assert not ops.detection_loss_large_route(65537) and not ops.detection_loss_large_route(0)


def _call(h, N, C, null=(), batch=2):
    """The entry with plausible host addresses (it must answer before it touches any of them)."""
    raw = ctypes.create_string_buffer(64 + 16)
    p = (ctypes.addressof(raw) + 15) & ~15
    args = [p] * 8 + [batch, N, C, 0.25, 3.0] + [p] * 5
    for i in null:
        args[i] = None
    return getattr(h, ENTRY)(None, *args)


def test_arguments_are_validated_before_any_hip_call():
    from egtr_amd import _lib
    h = _lib.lib()
    assert _call(h, 100, 5, null=(0,)) == -1                               # NULL logits
    assert _call(h, 65537, 5, null=(0,)) == -1                             # ... comes first
    for missing in ((13,), (14,), (15,), (13, 14), (14, 15), (13, 15)):   # some but not all gradients
        assert _call(h, 100, 5, null=missing) == -1
    assert _call(h, 100, 5, null=(16,)) == -1 and _call(h, 100, 5, null=(17,)) == -1   # out, workspace
    assert _call(h, 0, 5) == -1 and _call(h, 100, 0) == -1 and _call(h, 100, 5, batch=0) == -1
    assert _call(h, 65537, 5) == -3
    assert _call(h, 65537, 5, null=(13, 14, 15)) == -3                     # value-only: the same domain
    assert _call(h, 65537, 5, null=(5,)) == -3                             # class-agnostic: the same domain
    assert _call(h, 65536, 32768) == -3                                    # N * C = 2^31
    assert _call(h, 100, 5, batch=65536) == -3


def test_workspace_bytes_are_positive_and_monotone_over_the_served_range():
    from egtr_amd import _lib, ops
    q = getattr(_lib.lib(), QUERY)
    Rw = ops.DETECTION_LOSS_LARGE_ROWS
    sizes = sorted({1, Rw - 1, Rw, Rw + 1, 2048, 2049, 12537, 22223, 65535, 65536})
    got = [q(4, n, 150) for n in sizes]
    assert all(b > 0 for b in got) and got == sorted(got) and got[0] < got[-1]
    assert q(4, Rw, 150) < q(4, Rw + 1, 150)                               # a chunk more
    assert q(8, 12537, 150) == 2 * q(4, 12537, 150)
    assert q(4, 65536, 32767) > 0 and q(4, 65536, 32768) == 0              # N * C < 2^31
    for bad in ((4, 0, 150), (4, 65537, 150), (0, 100, 150), (4, 100, 0), (-1, 100, 5), (65536, 100, 5)):
        assert q(*bad) == 0, bad


# ------------------------------------------------------------------------------------------------ CPU tensors: routes
def _inputs(B, N, K, T, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, N, K, generator=g) * 3
    boxes = torch.cat([torch.rand(B, N, 2, generator=g) * 0.6 + 0.2, torch.rand(B, N, 2, generator=g) * 0.3 + 0.02], -1)
    targets = [{"class_labels": torch.randint(0, K, (T,), generator=g),
                "boxes": torch.cat([torch.rand(T, 2, generator=g) * 0.6 + 0.2, torch.rand(T, 2, generator=g) * 0.3 + 0.02], -1)}
               for _ in range(B)]
    return logits, boxes, targets


def _criteria():
    from egtr_amd.deformable_detr import DeformableDetrHungarianMatcher, DeformableDetrLoss
    from egtr_amd.egtr import SceneGraphGenerationLoss
    m = DeformableDetrHungarianMatcher(class_cost=2.0, bbox_cost=5.0, giou_cost=2.0, smoothing=1e-14)
    sgg = SceneGraphGenerationLoss(
        matcher=m, num_object_queries=20, num_classes=12, num_rel_labels=7, eos_coef=0.1,
        losses=["labels", "boxes", "cardinality"], smoothing=1e-14, rel_sample_negatives=80, rel_sample_nonmatching=80,
        model_training=True, focal_alpha=0.25, rel_sample_negatives_largest=True, rel_sample_nonmatching_largest=True)
    det = DeformableDetrLoss(m, 12, 0.1, ["labels", "boxes", "cardinality"], focal_alpha=0.25)
    return sgg, det


@pytest.mark.parametrize("which", ["scene_graph", "detection"])
def test_cpu_tensors_keep_the_composition_whatever_the_route_says(which, monkeypatch):
    """The two-stage criterion on CPU tensors: the same dict, bit for bit, with the route predicate as it is and answering
    False; neither the large op nor a launch is reached, nothing is counted in FALLBACKS."""
    from egtr_amd import _lib, ops
    logits, boxes, targets = _inputs(2, 20 if which == "scene_graph" else 2100, 12, 9, seed=3)
    enc_logits, enc_boxes, _ = _inputs(2, 2100, 12, 9, seed=4)
    out = {"logits": logits, "pred_boxes": boxes, "enc_outputs": {"logits": enc_logits, "pred_boxes": enc_boxes}}
    crit = _criteria()[0 if which == "scene_graph" else 1]

    def refuse(*a, **k):
        raise AssertionError("a CPU run reached the device route")
    monkeypatch.setattr(ops, "detection_losses_large", refuse)
    monkeypatch.setattr(_lib, "launch", refuse)
    fallbacks = dict(ops.FALLBACKS)
    as_is = crit(out, targets)
    monkeypatch.setattr(ops, "detection_loss_large_route", lambda n: False)
    forced = crit(out, targets)
    assert set(as_is) == set(forced) and {k for k in as_is if k.endswith("_enc")} == {
        "loss_ce_enc", "loss_bbox_enc", "loss_giou_enc", "cardinality_error_enc"}
    for k in as_is:
        assert torch.equal(as_is[k], forced[k]), k
    assert ops.FALLBACKS == fallbacks
    # ... and the values are the float64 restatement's on the criterion's own (host) assignment of the zero-label targets.
    # Bar: the composition sums 2 x 2100 x 12 fp32 terms pairwise (relative error of order 1e-6); 1e-4 max(1, |v|) is far from
    # any wrong term and two orders above that.
    import loss_restated as LR
    bin_targets = [dict(t, class_labels=torch.zeros_like(t["class_labels"])) for t in targets]
    indices, _ = crit.matcher(out["enc_outputs"], bin_targets)
    want = LR.detection_expectation(enc_logits, enc_boxes, indices, bin_targets, 0.25, 18.0,
                                    {"loss_ce": 2.0, "loss_bbox": 5.0, "loss_giou": 2.0})[0]
    for k, v in want.items():
        got = float(as_is[k + "_enc"])
        assert abs(got - v) < 1e-4 * max(1.0, abs(v)), (k, got, v)
