"""GPU (-m gpu): the device matcher for proposal-sized query sets (egtr_hungarian_match_large_f32, csrc/matcher.hip) --
the two-stage variant matches every encoder token against the class-agnostic targets.

Solve-only runs (``cost_in``) are held against scipy.optimize.linear_sum_assignment on the same float32 matrix: indices
array_equal in scipy's order, the matching costs bit-equal to the chosen entries, status 0.  Every case calls the large entry
directly (``large=True``; the entry accepts any N > T, so its edges are reached at small sizes).  Then the refusal paths, the
one-wave entry on the same inputs, the matcher module and the criterion's ``*_enc`` terms on the device against their CPU
(host route) runs, and the absence of a host synchronisation."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment as sp

import matcher_large_cases as MC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def solve(mats, large=True):
    from egtr_amd.ops import hungarian_match
    pi, ti, mc, n_out, status = hungarian_match(None, None, None, 1, 1, 1, cost_in=[torch.from_numpy(m).to(DEV) for m in mats],
                                                want_status=True, large=large)
    return pi.cpu().numpy(), ti.cpu().numpy(), mc.cpu().numpy(), n_out, status.cpu().numpy()


def assert_equals_scipy(mats, got, skip=()):
    pi, ti, mc, n_out, status = got
    o = 0
    for b, (m, n) in enumerate(zip(mats, n_out)):
        if b not in skip:
            a, c = sp(m)
            assert n == len(a) and status[b] == 0, (b, m.shape, status[b])
            assert np.array_equal(pi[o:o + n], a) and np.array_equal(ti[o:o + n], c), (b, m.shape)
            assert np.array_equal(mc[o:o + n].view(np.int32), m[a, c].view(np.int32)), (b, m.shape)
        o += n


@pytest.mark.parametrize("N,T", [(65, 1), (130, 5), (1025, 3), (1100, 5), (4099, 64), (12537, 30)])
def test_generic_costs_equal_scipy(N, T):
    """One column beyond a wave; the scan's remainder against 1024 threads (1025, 1100); several strides per thread; the
    workload's own size."""
    mats = [MC.generic(N, T)]
    assert_equals_scipy(mats, solve(mats))


@pytest.mark.parametrize("build", [c[1] for c in MC.TIE_CASES + MC.DUPLICATED_CASES],
                         ids=[c[0] for c in MC.TIE_CASES + MC.DUPLICATED_CASES])
def test_tied_costs_equal_scipy(build):
    """Ties in every scan: the (spc, unassigned first, position in ``remaining``) order decides, across waves too."""
    mats = [build()]
    assert_equals_scipy(mats, solve(mats))


def test_infinite_entries_that_leave_the_problem_feasible():
    rng = np.random.default_rng(11)
    m = MC.generic(1100, 5)
    m[rng.random(m.shape) < 0.3] = np.inf
    m[:7, 2] = np.inf
    assert np.isfinite(m).any(0).all()
    assert_equals_scipy([m], solve([m]))


def test_a_target_without_a_finite_cost_is_infeasible():
    m = MC.generic(1100, 5)
    m[:, 3] = np.inf
    with pytest.raises(ValueError):
        sp(m)
    pi, ti, mc, n_out, status = solve([m])
    assert n_out == [5] and status[0] == 2
    assert (pi == -1).all() and (ti == -1).all()


def test_ragged_batch_refuses_only_the_invalid_image():
    """T = 0, 1, 17, 40 in one launch; a NaN in the T = 17 image refuses that image alone."""
    N = 1300
    mats = [MC.generic(N, T, seed=40 + T) for T in (0, 1, 17, 40)]
    assert_equals_scipy(mats, solve(mats))
    mats[2][700, 9] = np.nan
    got = solve(mats)
    pi, ti, mc, n_out, status = got
    assert n_out == [0, 1, 17, 40] and list(status) == [0, 0, 1, 0]
    assert (pi[1:18] == -1).all() and (ti[1:18] == -1).all()
    assert_equals_scipy(mats, got, skip=(2,))


def test_invalid_entries_write_nothing_out_of_bounds():
    """A NaN image and a -inf image between two healthy ones, launched on buffers of this test's own: status 1 and -1 rows for
    the two, scipy's result for the others, and the canary words around every output slice and behind the workspace intact."""
    from egtr_amd import _lib
    N, Ts = 1100, (5, 7, 3, 6)
    B = len(Ts)
    mats = [MC.generic(N, T, seed=90 + T) for T in Ts]
    mats[1][1050, 4] = np.nan
    mats[2][3, 0] = -np.inf
    offs = np.concatenate([[0], np.cumsum(Ts)]).astype(np.int32)
    total, pad = int(offs[-1]), 8
    meta = torch.from_numpy(np.concatenate([offs, offs + pad])).to(DEV)     # outputs start `pad` words into their buffers
    cin = torch.cat([torch.from_numpy(m).reshape(-1) for m in mats]).to(DEV)
    pred = torch.full((total + 2 * pad,), 7777, dtype=torch.int64, device=DEV)
    tgt = torch.full((total + 2 * pad,), 8888, dtype=torch.int64, device=DEV)
    cost = torch.full((total + 2 * pad,), 99.0, dtype=torch.float32, device=DEV)
    status = torch.full((B + 2,), 55, dtype=torch.int32, device=DEV)
    n_ws = _lib.lib().egtr_hungarian_match_large_workspace_bytes(B, N, max(Ts), total)
    ws = torch.full((n_ws + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    _lib.launch("egtr_hungarian_match_large_f32", None, None, None, None, meta.data_ptr(), meta.data_ptr() + 4 * (B + 1), B, N,
                0, max(Ts), 1.0, 1.0, 1.0, 0, 0.0, 0.0, pred.data_ptr(), tgt.data_ptr(), cost.data_ptr(), None, cin.data_ptr(),
                status.data_ptr() + 4, ws.data_ptr(), n_ws)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [55, 0, 1, 1, 0, 55]
    assert (ws[n_ws:] == 0x5A).all()
    for buf, canary in ((pred, 7777), (tgt, 8888), (cost, 99.0)):
        assert (buf[:pad] == canary).all() and (buf[pad + total:] == canary).all()
    p, t, c = pred[pad:pad + total].cpu().numpy(), tgt[pad:pad + total].cpu().numpy(), cost[pad:pad + total].cpu().numpy()
    for b in (1, 2):
        assert (p[offs[b]:offs[b + 1]] == -1).all() and (t[offs[b]:offs[b + 1]] == -1).all()
    assert_equals_scipy(mats, (p, t, c, list(Ts), status[1:-1].cpu().numpy()), skip=(1, 2))


def test_a_workspace_too_small_for_the_batch_refuses_the_images_that_do_not_fit():
    """The host check can only hold the workspace against the smallest batch with this max_targets; an image whose cost
    block would end past the stated size is refused by the kernel (status 2) and the bytes behind that size stay untouched."""
    from egtr_amd import _lib
    N, Ts = 1100, (5, 5)
    mats = [MC.generic(N, T, seed=60 + i) for i, T in enumerate(Ts)]
    offs = np.array([0, 5, 10], dtype=np.int32)
    meta = torch.from_numpy(np.concatenate([offs, offs])).to(DEV)
    cin = torch.cat([torch.from_numpy(m).reshape(-1) for m in mats]).to(DEV)
    pred = torch.zeros(10, dtype=torch.int64, device=DEV)
    tgt = torch.zeros(10, dtype=torch.int64, device=DEV)
    cost = torch.zeros(10, dtype=torch.float32, device=DEV)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    q = _lib.lib().egtr_hungarian_match_large_workspace_bytes
    small, full = q(2, N, 5, 5), q(2, N, 5, 10)
    ws = torch.full((full,), 0x5A, dtype=torch.uint8, device=DEV)
    _lib.launch("egtr_hungarian_match_large_f32", None, None, None, None, meta.data_ptr(), meta.data_ptr() + 12, 2, N, 0, 5, 1.0,
                1.0, 1.0, 0, 0.0, 0.0, pred.data_ptr(), tgt.data_ptr(), cost.data_ptr(), None, cin.data_ptr(), status.data_ptr(),
                ws.data_ptr(), small)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 2]
    assert (ws[small:] == 0x5A).all()
    assert (pred[5:] == -1).all() and (tgt[5:] == -1).all()
    a, c = sp(mats[0])
    assert np.array_equal(pred[:5].cpu().numpy(), a) and np.array_equal(tgt[:5].cpu().numpy(), c)


def _real_inputs(B, N, K, T, seed, padded=0):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, N, K, generator=g) * 3
    boxes = torch.cat([torch.rand(B, N, 2, generator=g) * 0.6 + 0.2, torch.rand(B, N, 2, generator=g) * 0.3 + 0.02], -1)
    if padded:                                   # padded encoder tokens: equal logits, box (1, 1, 1, 1)
        logits[:, N - padded:] = -4.0
        boxes[:, N - padded:] = 1.0
    targets = [{"class_labels": torch.randint(0, K, (T,), generator=g),
                "boxes": torch.cat([torch.rand(T, 2, generator=g) * 0.6 + 0.2, torch.rand(T, 2, generator=g) * 0.3 + 0.02], -1)}
               for _ in range(B)]
    return logits, boxes, targets


def _to_dev(targets):
    return [{k: v.to(DEV) for k, v in t.items()} for t in targets]


def test_both_entries_agree_bit_for_bit_up_to_1024_queries():
    """The same inputs at N <= 1024 through egtr_hungarian_match_f32 and through the large entry: solve-only on generic, tied
    and refused matrices, and the fused cost evaluation (cost blocks included), with and without the smoothing offset."""
    from egtr_amd.ops import hungarian_match
    mats = [MC.generic(1024, 40), MC.tied_integers(700, 33, 3), MC.all_equal(200, 30), MC.padded_tokens(900, 64),
            MC.generic(65, 1), MC.tied_integers(1000, 90, 2, True)]
    bad = MC.generic(300, 8)
    bad[5, 5] = np.nan
    for group in ([mats[0]], [mats[1]], [mats[2]], [mats[3]], [mats[4]], [mats[5]], [bad]):
        small, large = solve(group, large=False), solve(group, large=True)
        for s, l in zip(small, large):
            assert np.array_equal(np.asarray(s), np.asarray(l))
    logits, boxes, targets = _real_inputs(3, 300, 7, 12, seed=21, padded=40)
    for cm, iss in ((None, None), (-17.5, 32.2)):
        outs = [hungarian_match(logits.to(DEV), boxes.to(DEV), _to_dev(targets), 2.0, 5.0, 2.0, cm, iss, want_cost=True,
                                want_status=True, large=flag) for flag in (False, True)]
        for k in (0, 1, 2, 5):
            assert torch.equal(outs[0][k], outs[1][k]), k
        assert outs[0][3] == outs[1][3]
        for x, y in zip(outs[0][4], outs[1][4]):
            assert torch.equal(x, y)


@pytest.mark.parametrize("smoothing", [0.0, 1e-14])
def test_matcher_module_takes_the_device_route_for_proposal_sized_sets(smoothing):
    """N = 1500 proposals, K = 1, 12 boxes per image through DeformableDetrHungarianMatcher: the device route, CUDA index
    tensors, the indices of the same matcher on CPU copies (host route: tensor composition + scipy) and its matching costs
    within the 1e-3 of the small-N device-matcher test (tests/test_gpu_model.py)."""
    from egtr_amd.deformable_detr import DeformableDetrHungarianMatcher
    logits, boxes, targets = _real_inputs(2, 1500, 1, 12, seed=3)
    m = DeformableDetrHungarianMatcher(class_cost=2.0, bbox_cost=5.0, giou_cost=2.0, smoothing=smoothing)
    host = m.prepare({"logits": logits, "pred_boxes": boxes}, targets)
    assert host[0] == "host"
    idx_ref, cost_ref = m.finish(host)
    out = {"logits": logits.to(DEV), "pred_boxes": boxes.to(DEV)}
    pending = m.prepare(out, _to_dev(targets))
    assert pending[0] == "device"
    idx, costs = m.finish(pending)
    assert int(idx.status.abs().sum()) == 0
    for (a, b), (ra, rb), c, rc in zip(idx, idx_ref, costs, cost_ref):
        assert a.is_cuda and b.is_cuda and c.is_cuda and a.dtype == torch.int64
        assert np.array_equal(a.cpu().numpy(), ra.numpy()) and np.array_equal(b.cpu().numpy(), rb.numpy())
        assert (c.cpu() - rc).abs().max() < 1e-3
    m.raise_if_invalid()


def _criterion(N, C, smoothing=1e-14):
    from egtr_amd.deformable_detr import DeformableDetrHungarianMatcher
    from egtr_amd.egtr import SceneGraphGenerationLoss
    m = DeformableDetrHungarianMatcher(class_cost=2.0, bbox_cost=5.0, giou_cost=2.0, smoothing=smoothing)
    return SceneGraphGenerationLoss(
        matcher=m, num_object_queries=N, num_classes=C, num_rel_labels=7, eos_coef=0.1,
        losses=["labels", "boxes", "cardinality"], smoothing=smoothing, rel_sample_negatives=80, rel_sample_nonmatching=80,
        model_training=True, focal_alpha=0.25, rel_sample_negatives_largest=True, rel_sample_nonmatching_largest=True)


ENC_TERMS = ("loss_ce_enc", "loss_bbox_enc", "loss_giou_enc", "cardinality_error_enc")


def _criterion_inputs(C=12):
    logits, boxes, targets = _real_inputs(2, 20, C, 12, seed=5)
    enc_logits, enc_boxes, _ = _real_inputs(2, 1500, C, 12, seed=6, padded=100)
    return logits, boxes, enc_logits, enc_boxes, targets


def test_criterion_enc_terms_equal_the_cpu_run():
    """SceneGraphGenerationLoss with ``enc_outputs`` of 1500 proposals: the ``*_enc`` terms of the CPU run (host route) within
    the tolerance of test_two_stage_model_vs_reference, 1e-3 * max(1, |v|)."""
    from egtr_amd.deformable_detr import DeformableDetrHungarianMatcher as Matcher
    logits, boxes, enc_logits, enc_boxes, targets = _criterion_inputs()
    crit = _criterion(20, 12)
    want = crit({"logits": logits, "pred_boxes": boxes, "enc_outputs": {"logits": enc_logits, "pred_boxes": enc_boxes}}, targets)
    Matcher.raise_if_invalid()
    got = crit.to(DEV)({"logits": logits.to(DEV), "pred_boxes": boxes.to(DEV),
                        "enc_outputs": {"logits": enc_logits.to(DEV), "pred_boxes": enc_boxes.to(DEV)}}, _to_dev(targets))
    assert set(ENC_TERMS) <= set(got) and set(got) == set(want)
    for k in ENC_TERMS:
        v = float(want[k])
        assert got[k].is_cuda and abs(float(got[k]) - v) < 1e-3 * max(1.0, abs(v)), (k, float(got[k]), v)
    Matcher.raise_if_invalid()


def test_a_nan_proposal_box_poisons_the_enc_terms_and_raises_once():
    from egtr_amd.deformable_detr import DeformableDetrHungarianMatcher as Matcher
    logits, boxes, enc_logits, enc_boxes, targets = _criterion_inputs()
    enc_boxes[1, 1234, 2] = float("nan")
    Matcher.raise_if_invalid()                       # drain what earlier tests left behind
    got = _criterion(20, 12).to(DEV)({"logits": logits.to(DEV), "pred_boxes": boxes.to(DEV),
                                      "enc_outputs": {"logits": enc_logits.to(DEV), "pred_boxes": enc_boxes.to(DEV)}},
                                     _to_dev(targets))
    torch.cuda.synchronize()
    for k in ENC_TERMS:
        assert torch.isnan(got[k]).item(), k
    for k in ("loss_ce", "loss_bbox", "loss_giou"):
        assert torch.isfinite(got[k]).item(), k       # the main output set was matched
    with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
        Matcher.raise_if_invalid()
    Matcher.raise_if_invalid()                       # reported once


def test_matcher_call_on_proposals_does_not_synchronise():
    """The whole matcher on N = 1500 inputs is enqueued: cost block, assignment, status copy -- no host wait."""
    from egtr_amd.deformable_detr import DeformableDetrHungarianMatcher
    logits, boxes, targets = _real_inputs(2, 1500, 1, 12, seed=8)
    m = DeformableDetrHungarianMatcher(class_cost=2.0, bbox_cost=5.0, giou_cost=2.0, smoothing=1e-14)
    out, dt = {"logits": logits.to(DEV), "pred_boxes": boxes.to(DEV)}, _to_dev(targets)
    first, _ = m(out, dt)          # first call: the pinned status buffers are allocated outside the checked region
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        idx, costs = m(out, dt)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for (a, b), (fa, fb) in zip(idx, first):
        assert a.is_cuda and torch.equal(a, fa) and torch.equal(b, fb)
    m.raise_if_invalid()
