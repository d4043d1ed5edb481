"""GPU (-m gpu): the detection losses of a proposal-sized output set (csrc/loss.hip, det_loss_large_f32 + det_loss_large_sum:
a workgroup per ``Rw`` query rows of an image, then the per-image sums) against oracle.loss.labels_boxes_card in float64 under
autograd (tests/loss_restated.py), with the matches SUPPLIED: sizes around the rows-per-workgroup constant and the limits of the
entry, matches on chunk edges, every branch of the shared box term, skipped match entries, class-agnostic targets, the
value-only launch, bit-reproducibility, refusals, the absence of a host wait and the routes of the two criteria.

Bars (those of tests/test_gpu_detection_loss_edges.py; the per-thread fp32 partial sums of this kernel are shorter than the
one-workgroup kernel's at N = 2048, C = 150): values 2e-5 max(1, |ref|), gradients 2e-5 max(1e-3, max|grad_ref|)."""
import numpy as np
import pytest
import torch

import loss_restated as LR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WEIGHTS = {"loss_ce": 2.0, "loss_bbox": 5.0, "loss_giou": 2.0}
KEYS = ("loss_ce", "loss_bbox", "loss_giou", "cardinality_error")
ENTRY = "egtr_detection_loss_large_f32"


Rw = 32     # the parametrize lists are built at import: pinned to the binding's constant by the test below


def test_the_rows_per_workgroup_here_are_the_bindings():
    from egtr_amd import ops
    assert ops.DETECTION_LOSS_LARGE_ROWS == Rw


def flat_match(indices):
    return (torch.cat([s for s, _ in indices]).to(DEV), torch.cat([t for _, t in indices]).to(DEV),
            [int(s.shape[0]) for s, _ in indices])


def kernel_losses(logits, boxes, indices, targets, focal_alpha, num_boxes, class_agnostic=False):
    """ops.detection_losses_large with the given matches -> (losses as floats, d total / d logits, d total / d boxes,
    d loss_bbox / d boxes, d loss_giou / d boxes) on the host."""
    from egtr_amd import ops
    lg = logits.to(DEV).requires_grad_(True)
    bx = boxes.to(DEV).requires_grad_(True)
    packed = ops.pack_detection_targets([{k: v.to(DEV) for k, v in t.items()} for t in targets], DEV)
    losses = ops.detection_losses_large(lg, bx, flat_match(indices), packed, focal_alpha, num_boxes, class_agnostic)
    total = sum(losses[k] * w for k, w in WEIGHTS.items())
    g_lg, g_bx = torch.autograd.grad(total, [lg, bx], retain_graph=True)
    g_l1, = torch.autograd.grad(losses["loss_bbox"], bx, retain_graph=True)
    g_giou, = torch.autograd.grad(losses["loss_giou"], bx)
    torch.cuda.synchronize()
    return {k: float(v.detach()) for k, v in losses.items()}, g_lg.cpu(), g_bx.cpu(), g_l1.cpu(), g_giou.cpu()


def compare(tag, got, want, gradients=True):
    """Prints every figure, then asserts the bars.  Returns the largest error / bar."""
    worst = 0.0
    assert set(got[0]) == set(KEYS)
    for k in KEYS:
        err, bar = abs(got[0][k] - want[0][k]), 2e-5 * max(1.0, abs(want[0][k]))
        print(f"{tag}: {k} {got[0][k]:.7g} vs {want[0][k]:.7g}: err {err:.3e} (bar {bar:.3e})")
        worst = max(worst, err / bar)
        assert err < bar, (tag, k)
    if gradients:
        for what, g, r in zip(("d logits", "d boxes", "d bbox / d boxes", "d giou / d boxes"), got[1:], want[1:]):
            err, bar = float((g.double() - r).abs().max()), 2e-5 * max(1e-3, float(r.abs().max()))
            print(f"{tag}: {what}: err {err:.3e} (bar {bar:.3e})")
            worst = max(worst, err / bar)
            assert err < bar, (tag, what)
    return worst


def random_batch(seed, N, C, Ts):
    """Random logits / boxes / targets and RANDOM one-to-one matches (unsorted, as no matcher would refuse)."""
    rng = np.random.default_rng(seed)
    B = len(Ts)
    logits = torch.as_tensor((rng.standard_normal((B, N, C)) * 2).astype(np.float32))
    box = lambda *lead: np.concatenate([rng.uniform(0.2, 0.8, (*lead, 2)), rng.uniform(0.05, 0.4, (*lead, 2))], -1)  # noqa: E731
    boxes = torch.as_tensor(box(B, N).astype(np.float32))
    targets = [{"class_labels": torch.as_tensor(rng.integers(0, C, t)).long(), "boxes": torch.as_tensor(box(t).astype(np.float32))}
               for t in Ts]
    indices = [(torch.as_tensor(rng.permutation(N)[:t]).long(), torch.as_tensor(rng.permutation(t)).long()) for t in Ts]
    return logits, boxes, indices, targets


def n_boxes(targets):
    return max(float(sum(len(t["class_labels"]) for t in targets)), 1.0)


def both(tag, logits, boxes, indices, targets, focal_alpha=0.25, gradients=True, oracle_indices=None):
    """``oracle_indices``: what the expectation is built from when the kernel's own list holds entries it has to skip."""
    got = kernel_losses(logits, boxes, indices, targets, focal_alpha, n_boxes(targets))
    want = LR.detection_expectation(logits, boxes, oracle_indices if oracle_indices is not None else indices, targets,
                                    focal_alpha, n_boxes(targets), WEIGHTS)
    return got, want, compare(tag, got, want, gradients)


def raw_launch(logits, boxes, indices, targets, grads="all", class_agnostic=False, fill=float("nan"), num_boxes=None):
    """The C entry called directly on NaN-filled outputs: (status, out, d_logits, d_l1, d_giou).  ``grads``: "all", "none" or
    the index of the one gradient pointer that is NULL."""
    from egtr_amd import _lib, ops
    lg, bx = logits.to(DEV).contiguous(), boxes.to(DEV).contiguous()
    B, N, C = lg.shape
    labels, tboxes, toff, _ = ops.pack_detection_targets([{k: v.to(DEV) for k, v in t.items()} for t in targets], DEV)
    pi, ti, n_out = flat_match(indices)
    if pi.numel() == 0:
        pi = ti = torch.zeros(1, dtype=torch.int64, device=DEV)
    moff = torch.tensor(np.concatenate([[0], np.cumsum(n_out)]), dtype=torch.int32).to(DEV)
    n_ws = _lib.lib().egtr_detection_loss_large_workspace_bytes(B, N, C)
    assert n_ws > 0
    ws = torch.empty((n_ws + 7) // 8, dtype=torch.float64, device=DEV)
    out = torch.full((B, 4), fill, device=DEV)
    g = [torch.full_like(lg, fill), torch.full_like(bx, fill), torch.full_like(bx, fill)]
    ptrs = [t.data_ptr() for t in g]
    if grads == "none":
        ptrs = [None, None, None]
    elif grads != "all":
        ptrs[grads] = None
    st = getattr(_lib.lib(), ENTRY)(_lib._stream(), lg.data_ptr(), bx.data_ptr(), pi.data_ptr(), ti.data_ptr(), moff.data_ptr(),
                                    None if class_agnostic else labels.data_ptr(), tboxes.data_ptr(), toff.data_ptr(), B, N, C,
                                    0.25, float(num_boxes or n_boxes(targets)), *ptrs, out.data_ptr(), ws.data_ptr())
    torch.cuda.synchronize()
    return st, out.cpu(), g[0].cpu(), g[1].cpu(), g[2].cpu()


# -------------------------------------------------------------------------------------------------------------- sizes
REAL_SHAPE = (12537, 150, (26, 13))


@pytest.mark.parametrize("N,C,Ts", [(1, 1, (1,)), (Rw - 1, 5, (9, 0, 4)), (Rw, 5, (9, 0, 4)), (Rw + 1, 5, (9, 0, 4)),
                                    (2049, 5, (1500, 0, 7)), (4100, 150, (9, 0, 4)), REAL_SHAPE, (65536, 2, (300, 0)),
                                    (2 * Rw + 3, 1, (9, 0, 4)), (2 * Rw + 3, 64, (9, 0, 4)), (2 * Rw + 3, 65, (9, 0, 4)),
                                    (2 * Rw + 3, 150, (9, 0, 4))])
def test_sizes(N, C, Ts):
    """One row; a last chunk of Rw - 1, Rw and 1 rows; the first size the one-workgroup entry refuses, with more matches in an
    image (1500) than a workgroup has threads; the real proposal count; the largest N served; C = 1, a full 64-lane trip, a
    second trip with one live lane and a ragged third one.  Images without a target: labels only, box gradients exactly zero."""
    logits, boxes, indices, targets = random_batch(9000 + N + C, N, C, Ts)
    got, want, worst = both(f"sizes N={N} C={C}", logits, boxes, indices, targets)
    for b, t in enumerate(Ts):
        if t == 0:
            assert float(got[1][b].abs().max()) > 0 and float(got[2][b].abs().max()) == 0.0
    print(f"sizes N={N} C={C}: worst err / bar {worst:.3f}")


@pytest.mark.parametrize("C", [5, 65, 150])
def test_cardinality_argmax_ties(C):
    """The first maximum wins: ties that include the last class, ties inside one lane's strided share (c and c + 64), all-equal
    rows, a unique maximum in the last class -- on rows of both chunks; the per-image counts straight from the launch."""
    N = Rw + 40
    logits, boxes, indices, targets = random_batch(6100 + C, N, C, (6, 0, 3))
    ties = [[1, C - 1], [C - 2, C - 1], [0, C - 1], [C - 1]]
    if C > 64:
        ties += [[0, 64], [63, 64], [C - 65, C - 1], [5, min(64 + 5, C - 2), C - 1]]
    if C > 128:
        ties += [[70, 149], [5, 69, 133], [21, 149], [127, 128]]
    want_cnt = []
    for b in range(3):
        for i, cls in enumerate(ties):
            logits[b, Rw - 6 + 3 * i + b, cls] = 9.0 + i                   # above every random logit; rows on both sides of Rw
        logits[b, 3] = -1.25                                              # all equal
        logits[b, N - 2] = 0.0
        logits[b, N - 1] = -3.0
        logits[b, N - 1, C - 1] = -2.0                                    # unique maximum: the last class, low values
        want_cnt.append(int((logits[b].numpy().argmax(-1) != C - 1).sum()))
    both(f"cardinality C={C}", logits, boxes, indices, targets)
    st, out, _, _, _ = raw_launch(logits, boxes, indices, targets)
    print("cardinality C =", C, "counts", out[:, 3].tolist(), "want", want_cnt)
    assert st == 0 and out[:, 3].tolist() == [float(c) for c in want_cnt]
    assert all(0 < c <= N - 2 for c in want_cnt)                           # some rows DO end in the last class


# -------------------------------------------------------------------------------------------------------- chunk edges
def edge_batch():
    """N = 2 Rw + 3 (three chunks, the last of 3 rows): image 0 matched on the first and last row of every chunk, image 1 with all
    of its matches inside the middle chunk, image 2 without targets."""
    N = 2 * Rw + 3
    logits, boxes, indices, targets = random_batch(4242, N, 7, (5, 8, 0))
    indices[0] = (torch.tensor([Rw, 0, N - 1, Rw - 1, 2 * Rw - 1]), indices[0][1])
    indices[1] = (torch.tensor([Rw + 3, Rw + 9, Rw + 4, 2 * Rw - 2, Rw + 1, Rw + 14, Rw + 15, Rw + 17]), indices[1][1])
    assert len(set(indices[1][0].tolist())) == 8 and all(Rw <= r < 2 * Rw for r in indices[1][0].tolist())
    return logits, boxes, indices, targets


def test_matches_on_chunk_edges():
    logits, boxes, indices, targets = edge_batch()
    got, want, worst = both("chunk edges", logits, boxes, indices, targets)
    for b in (0, 1):                                                       # every matched row received its L1 gradient
        assert bool((got[3][b, indices[b][0]].abs().sum(-1) > 0).all())
    print(f"chunk edges: worst err / bar {worst:.3f}")


def test_unmatched_rows_of_the_box_gradients_are_written_as_zeros():
    """NaN-filled buffers into a direct launch: every element is overwritten, unmatched rows with exactly 0.0."""
    logits, boxes, indices, targets = edge_batch()
    st, out, d_lg, d_l1, d_giou = raw_launch(logits, boxes, indices, targets)
    assert st == 0
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(d_lg).all())
    matched = torch.zeros(d_l1.shape[:2], dtype=torch.bool)
    for b, (rows, _) in enumerate(indices):
        matched[b, rows] = True
    for g in (d_l1, d_giou):
        assert bool(torch.isfinite(g).all())
        assert float(g[~matched].abs().max()) == 0.0 and bool((g[matched].abs().sum(-1) > 0).all())
    # a larger set: 1500 matches in one image, more than a workgroup has threads
    logits, boxes, indices, targets = random_batch(11, 2049, 5, (1500, 0, 7))
    st, out, d_lg, d_l1, d_giou = raw_launch(logits, boxes, indices, targets)
    matched = torch.zeros(d_l1.shape[:2], dtype=torch.bool)
    for b, (rows, _) in enumerate(indices):
        matched[b, rows] = True
    assert st == 0 and bool(torch.isfinite(d_lg).all())
    for g in (d_l1, d_giou):
        assert bool(torch.isfinite(g).all()) and float(g[~matched].abs().max()) == 0.0
        assert bool((g[matched].abs().sum(-1) > 0).all())


# ------------------------------------------------------------------------------------------------- box configurations
# (cx, cy, w, h) of the prediction and of its target; no two compared corner coordinates are equal except in "identical"
BOXES = {
    "disjoint_x": ((0.2, 0.5, 0.2, 0.3), (0.7, 0.52, 0.22, 0.36)),
    "disjoint_y": ((0.5, 0.2, 0.3, 0.2), (0.52, 0.7, 0.36, 0.22)),
    "disjoint_both": ((0.2, 0.2, 0.2, 0.22), (0.7, 0.75, 0.25, 0.3)),
    "prediction_inside": ((0.5, 0.52, 0.1, 0.12), (0.48, 0.5, 0.4, 0.5)),
    "target_inside": ((0.48, 0.5, 0.4, 0.5), (0.5, 0.52, 0.1, 0.12)),
    "overlap_upper_right": ((0.4, 0.4, 0.3, 0.32), (0.5, 0.52, 0.28, 0.34)),
    "overlap_upper_left": ((0.4, 0.4, 0.3, 0.32), (0.3, 0.52, 0.28, 0.34)),
    "overlap_lower_right": ((0.4, 0.4, 0.3, 0.32), (0.5, 0.28, 0.28, 0.34)),
    "overlap_lower_left": ((0.4, 0.4, 0.3, 0.32), (0.3, 0.28, 0.28, 0.34)),
    "thin": ((0.5, 0.5, 0.02, 0.4), (0.507, 0.48, 0.03, 0.5)),
    "identical": ((0.4, 0.6, 0.3, 0.2), (0.4, 0.6, 0.3, 0.2)),
}


@pytest.mark.parametrize("name", list(BOXES))
def test_giou_gradient_branches(name):
    """One matched pair (query 2 of 4) per configuration through the shared box term."""
    pred, tgt = BOXES[name]
    logits, boxes, _, _ = random_batch(77, 4, 6, (1,))
    boxes[0, 2] = torch.tensor(pred)
    targets = [{"class_labels": torch.tensor([3]), "boxes": torch.tensor([tgt], dtype=torch.float32)}]
    indices = [(torch.tensor([2]), torch.tensor([0]))]
    got, want, worst = both(f"boxes {name}", logits, boxes, indices, targets, gradients=name != "identical")
    for g in got[3:]:
        assert float(g[0, [0, 1, 3]].abs().max()) == 0.0                 # unmatched queries: no box gradient
    if name == "identical":
        # min / max at exact ties: torch splits the gradient, the kernel takes one side -- both are subgradients
        assert got[0]["loss_bbox"] == 0.0 and abs(got[0]["loss_giou"]) < 2e-5
        assert float(got[3].abs().max()) == 0.0 and bool(torch.isfinite(got[4]).all()) and bool(torch.isfinite(got[2]).all())
    else:
        assert float(got[4][0, 2].abs().max()) > 0
    print(f"boxes {name}: worst err / bar {worst:.3f}")


def test_box_term_equals_the_one_workgroup_entry_bit_for_bit():
    """Both kernels call the same device functions: the same inputs through ops.detection_losses give the same gradients."""
    from egtr_amd import ops
    logits, boxes, indices, targets = random_batch(31, 2 * Rw + 3, 9, (12, 0, 5))
    big = kernel_losses(logits, boxes, indices, targets, 0.25, 17.0)
    lg, bx = logits.to(DEV).requires_grad_(True), boxes.to(DEV).requires_grad_(True)
    packed = ops.pack_detection_targets([{k: v.to(DEV) for k, v in t.items()} for t in targets], DEV)
    small = ops.detection_losses(lg, bx, flat_match(indices), packed, 0.25, 17.0)
    g_lg, = torch.autograd.grad(small["loss_ce"], lg, retain_graph=True)
    g_l1, = torch.autograd.grad(small["loss_bbox"], bx, retain_graph=True)
    g_giou, = torch.autograd.grad(small["loss_giou"], bx)
    assert torch.equal(g_l1.cpu(), big[3]) and torch.equal(g_giou.cpu(), big[4])
    assert torch.equal((g_lg * WEIGHTS["loss_ce"]).cpu(), big[1])
    assert float(small["cardinality_error"]) == big[0]["cardinality_error"]


# ----------------------------------------------------------------------------------------------------- skipped entries
def test_entries_with_an_index_out_of_range_are_skipped():
    """Image 1's prediction indices all -1 (a refused image): the expectation without that image's matches, its box gradients
    zero.  Prediction index N and target index T_b in image 0 are skipped as well."""
    N = 2 * Rw + 3
    logits, boxes, indices, targets = random_batch(515, N, 5, (6, 5, 4))
    empty = (torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    refused = [indices[0], (torch.full_like(indices[1][0], -1), torch.full_like(indices[1][1], -1)), indices[2]]
    got, want, worst = both("refused image", logits, boxes, refused, targets, oracle_indices=[indices[0], empty, indices[2]])
    assert float(got[2][1].abs().max()) == 0.0 and float(got[2][0].abs().max()) > 0
    full = LR.detection_expectation(logits, boxes, indices, targets, 0.25, n_boxes(targets), WEIGHTS)
    assert abs(full[0]["loss_bbox"] - want[0]["loss_bbox"]) > 1e-3          # the image's matches do count when present
    p0, t0 = indices[0][0].clone(), indices[0][1].clone()
    p0[1], t0[4] = N, 6                                                    # one past the last query, one past the last target
    keep = torch.tensor([0, 2, 3, 5])
    got, want, worst2 = both("index N, target T_b", logits, boxes, [(p0, t0), indices[1], indices[2]], targets,
                             oracle_indices=[(indices[0][0][keep], indices[0][1][keep]), indices[1], indices[2]])
    assert float(got[2][0, indices[0][0][[1, 4]]].abs().max()) == 0.0
    print(f"skipped entries: worst err / bar {max(worst, worst2):.3f}")


# ------------------------------------------------------------------------------------------------------ class-agnostic
def test_class_agnostic_equals_labels_of_zeros():
    logits, boxes, indices, targets = random_batch(616, 2 * Rw + 3, 12, (9, 0, 14))
    assert int(sum(int((t["class_labels"] != 0).sum()) for t in targets)) > 10
    zeros = [dict(t, class_labels=torch.zeros_like(t["class_labels"])) for t in targets]
    a = kernel_losses(logits, boxes, indices, targets, 0.25, 23.0, class_agnostic=True)
    z = kernel_losses(logits, boxes, indices, zeros, 0.25, 23.0)
    real = kernel_losses(logits, boxes, indices, targets, 0.25, 23.0)
    assert a[0] == z[0] and all(torch.equal(x, y) for x, y in zip(a[1:], z[1:]))
    assert a[0]["loss_ce"] != real[0]["loss_ce"] and not torch.equal(a[1], real[1])   # the labels do matter when they are read
    want = LR.detection_expectation(logits, boxes, indices, zeros, 0.25, 23.0, WEIGHTS)
    compare("class-agnostic", a, want)


# ---------------------------------------------------------------------------------------------------------- value-only
def test_value_only_launch(monkeypatch):
    from egtr_amd import ops
    logits, boxes, indices, targets = random_batch(717, 2 * Rw + 3, 12, (9, 0, 14))
    packed = ops.pack_detection_targets([{k: v.to(DEV) for k, v in t.items()} for t in targets], DEV)
    lg, bx = logits.to(DEV).requires_grad_(True), boxes.to(DEV).requires_grad_(True)
    with_grad = ops.detection_losses_large(lg, bx, flat_match(indices), packed, 0.25, 23.0)
    assert with_grad["loss_ce"].requires_grad
    launches = []
    real = ops.detection_loss_large_launch
    monkeypatch.setattr(ops, "detection_loss_large_launch",
                        lambda *a, **k: (launches.append(k.get("want_grad")), real(*a, **k))[1])
    with torch.no_grad():
        no_grad = ops.detection_losses_large(lg, bx, flat_match(indices), packed, 0.25, 23.0)
    detached = ops.detection_losses_large(lg.detach(), bx.detach(), flat_match(indices), packed, 0.25, 23.0)
    assert launches == [False, False]                                      # the value-only launch, no gradient buffers
    for k in KEYS:
        assert not no_grad[k].requires_grad and torch.equal(no_grad[k], with_grad[k].detach()), k
        assert torch.equal(detached[k], with_grad[k].detach()), k
    # the entry itself: three NULL gradients are the value-only launch, nothing but `out` is written; one NULL is an error
    st_all, out_all, _, _, _ = raw_launch(logits, boxes, indices, targets)
    st, out, d_lg, d_l1, d_giou = raw_launch(logits, boxes, indices, targets, grads="none")
    assert st_all == 0 and st == 0 and torch.equal(out, out_all)
    assert bool(torch.isnan(d_lg).all()) and bool(torch.isnan(d_l1).all()) and bool(torch.isnan(d_giou).all())
    for missing in (0, 1, 2):
        st, out, d_lg, d_l1, d_giou = raw_launch(logits, boxes, indices, targets, grads=missing)
        assert st == -1
        assert all(bool(torch.isnan(t).all()) for t in (out, d_lg, d_l1, d_giou))


# ----------------------------------------------------------------------------------------------------- reproducibility
def test_the_real_shape_gives_the_same_bits_five_times():
    N, C, Ts = REAL_SHAPE
    logits, boxes, indices, targets = random_batch(9000 + N + C, N, C, Ts)
    runs = [raw_launch(logits, boxes, indices, targets) for _ in range(5)]
    for r in runs[1:]:
        assert r[0] == 0 and all(torch.equal(x, y) for x, y in zip(r[1:], runs[0][1:]))


# ------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("N,C", [(65537, 1), (65536, 32768)])
def test_shapes_outside_the_domain_are_refused_before_any_launch(N, C):
    """Argument check only: every buffer holds one NaN-filled element, and keeps it."""
    from egtr_amd import _lib
    h = _lib.lib()
    assert h.egtr_detection_loss_large_workspace_bytes(2, N, C) == 0
    f = [torch.full((4,), float("nan"), device=DEV) for _ in range(7)]
    i64 = torch.zeros(2, dtype=torch.int64, device=DEV)
    i32 = torch.zeros(4, dtype=torch.int32, device=DEV)
    st = getattr(h, ENTRY)(_lib._stream(), f[0].data_ptr(), f[1].data_ptr(), i64.data_ptr(), i64.data_ptr(), i32.data_ptr(),
                           i64.data_ptr(), f[2].data_ptr(), i32.data_ptr(), 2, N, C, 0.25, 3.0, f[3].data_ptr(), f[4].data_ptr(),
                           f[5].data_ptr(), f[6].data_ptr(), f[6].data_ptr())
    torch.cuda.synchronize()
    assert st == -3
    assert all(bool(torch.isnan(t).all()) for t in f)
    if C == 1:      # the binding says so in words before it allocates anything
        from egtr_amd import ops
        with pytest.raises(_lib.EgtrHipError, match="serves 1 <= N <= 65536"):
            ops.detection_loss_large_launch(torch.zeros(1, N, 1, device=DEV), torch.zeros(1, N, 4, device=DEV), i64, i64, i32,
                                            None, f[2], i32, 0.25, 1.0)


# -------------------------------------------------------------------------------------------------------- no host wait
def test_the_op_does_not_wait_for_the_device():
    from egtr_amd import ops
    logits, boxes, indices, targets = random_batch(818, 2049, 5, (30, 0, 7))
    packed = ops.pack_detection_targets([{k: v.to(DEV) for k, v in t.items()} for t in targets], DEV)
    lg, bx, flat = logits.to(DEV).requires_grad_(True), boxes.to(DEV).requires_grad_(True), flat_match(indices)
    first = ops.detection_losses_large(lg, bx, flat, packed, 0.25, 37.0)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = ops.detection_losses_large(lg, bx, flat, packed, 0.25, 37.0)
        sum(second[k] * w for k, w in WEIGHTS.items()).backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert all(torch.equal(first[k], second[k]) for k in KEYS) and lg.grad is not None


# -------------------------------------------------------------------------------------------------------------- routes
ENC_TERMS = ("loss_ce_enc", "loss_bbox_enc", "loss_giou_enc", "cardinality_error_enc")


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


def _matcher(smoothing=1e-14):
    from egtr_amd.deformable_detr import DeformableDetrHungarianMatcher
    return DeformableDetrHungarianMatcher(class_cost=2.0, bbox_cost=5.0, giou_cost=2.0, smoothing=smoothing)


def _sgg_criterion(N, C, losses=("labels", "boxes", "cardinality")):
    from egtr_amd.egtr import SceneGraphGenerationLoss
    return SceneGraphGenerationLoss(
        matcher=_matcher(), num_object_queries=N, num_classes=C, num_rel_labels=7, eos_coef=0.1, losses=list(losses),
        smoothing=1e-14, rel_sample_negatives=80, rel_sample_nonmatching=80, model_training=True, focal_alpha=0.25,
        rel_sample_negatives_largest=True, rel_sample_nonmatching_largest=True)


def _criterion_inputs(S=2500, C=12):
    logits, boxes, targets = _real_inputs(2, 20, C, 12, seed=5)
    enc_logits, enc_boxes, _ = _real_inputs(2, S, C, 12, seed=6, padded=100)
    return logits, boxes, enc_logits, enc_boxes, targets


@pytest.fixture
def launches(monkeypatch):
    """The names of the entries launched through _lib.launch, in order."""
    from egtr_amd import _lib
    names, real = [], _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    return names


def _enc_total(d):
    return 2.0 * d["loss_ce_enc"] + 5.0 * d["loss_bbox_enc"] + 2.0 * d["loss_giou_enc"]


def test_scene_graph_criterion_routes_the_proposal_set_through_the_large_entry(launches, monkeypatch):
    from egtr_amd import ops
    from egtr_amd.deformable_detr import DeformableDetrHungarianMatcher as Matcher
    logits, boxes, enc_logits, enc_boxes, targets = _criterion_inputs()
    crit = _sgg_criterion(20, 12)
    el, eb = enc_logits.clone().requires_grad_(True), enc_boxes.clone().requires_grad_(True)
    want = crit({"logits": logits, "pred_boxes": boxes, "enc_outputs": {"logits": el, "pred_boxes": eb}}, targets)
    want_g = torch.autograd.grad(_enc_total(want), [el, eb])
    Matcher.raise_if_invalid()
    assert ENTRY not in launches                                            # CPU tensors: the composition
    fallbacks = dict(ops.FALLBACKS)
    crit = crit.to(DEV)
    calls, real_get_loss = [], crit.get_loss
    monkeypatch.setattr(crit, "get_loss", lambda loss, out, *a, **k: (calls.append((loss, out["logits"].shape[1])),
                                                                      real_get_loss(loss, out, *a, **k))[1])
    dl, db = enc_logits.to(DEV).requires_grad_(True), enc_boxes.to(DEV).requires_grad_(True)
    got = crit({"logits": logits.to(DEV), "pred_boxes": boxes.to(DEV), "enc_outputs": {"logits": dl, "pred_boxes": db}},
               _to_dev(targets))
    got_g = torch.autograd.grad(_enc_total(got), [dl, db])
    torch.cuda.synchronize()
    Matcher.raise_if_invalid()
    assert launches.count(ENTRY) == 1 and launches.count("egtr_detection_loss_f32") == 1
    assert not [c for c in calls if c[1] == enc_logits.shape[1]], calls      # no composition for the proposal set
    assert set(got) == set(want) and ops.FALLBACKS == fallbacks
    for k in ENC_TERMS:
        v = float(want[k])
        print(k, float(got[k]), v)
        assert got[k].is_cuda and abs(float(got[k]) - v) < 1e-3 * max(1.0, abs(v)), (k, float(got[k]), v)
    for what, g, r in zip(("d enc_logits", "d enc_boxes"), got_g, want_g):
        err, bar = float((g.cpu().double() - r.double()).abs().max()), 2e-5 * max(1e-3, float(r.abs().max()))
        print(f"{what}: err {err:.3e} (bar {bar:.3e})")
        assert err < bar, what


def test_detection_criterion_routes_both_large_sets_and_packs_once(launches, monkeypatch):
    from egtr_amd import ops
    from egtr_amd.deformable_detr import DeformableDetrHungarianMatcher as Matcher, DeformableDetrLoss
    logits, boxes, targets = _real_inputs(2, 2500, 12, 12, seed=15)
    enc_logits, enc_boxes, _ = _real_inputs(2, 2500, 12, 12, seed=16, padded=100)
    crit = DeformableDetrLoss(_matcher(), 12, 0.1, ["labels", "boxes", "cardinality"], focal_alpha=0.25)
    want = crit({"logits": logits, "pred_boxes": boxes, "enc_outputs": {"logits": enc_logits, "pred_boxes": enc_boxes}}, targets)
    Matcher.raise_if_invalid()
    assert ENTRY not in launches
    packs, real_pack = [], ops.pack_detection_targets
    monkeypatch.setattr(ops, "pack_detection_targets", lambda *a, **k: (packs.append(1), real_pack(*a, **k))[1])
    fallbacks = dict(ops.FALLBACKS)
    got = crit.to(DEV)({"logits": logits.to(DEV), "pred_boxes": boxes.to(DEV),
                        "enc_outputs": {"logits": enc_logits.to(DEV), "pred_boxes": enc_boxes.to(DEV)}}, _to_dev(targets))
    torch.cuda.synchronize()
    Matcher.raise_if_invalid()
    assert launches.count(ENTRY) == 2 and "egtr_detection_loss_f32" not in launches and len(packs) == 1
    assert set(got) == set(want) and ops.FALLBACKS == fallbacks
    for k, v in want.items():
        v = float(v)
        assert abs(float(got[k]) - v) < 1e-3 * max(1.0, abs(v)), (k, float(got[k]), v)


def test_bf16_logits_and_a_missing_term_keep_the_composition(launches):
    from egtr_amd import ops
    from egtr_amd.deformable_detr import DeformableDetrHungarianMatcher as Matcher
    logits, boxes, enc_logits, enc_boxes, targets = _criterion_inputs(S=300)
    fallbacks = dict(ops.FALLBACKS)
    out = {"logits": logits.to(DEV), "pred_boxes": boxes.to(DEV),
           "enc_outputs": {"logits": enc_logits.to(DEV).bfloat16(), "pred_boxes": enc_boxes.to(DEV)}}
    got = _sgg_criterion(20, 12).to(DEV)(out, _to_dev(targets))
    assert all(bool(torch.isfinite(got[k])) for k in ENC_TERMS)
    out["enc_outputs"]["logits"] = enc_logits.to(DEV)
    got = _sgg_criterion(20, 12, losses=("labels", "boxes")).to(DEV)(out, _to_dev(targets))    # no cardinality term
    assert "loss_ce_enc" in got and "cardinality_error_enc" not in got
    torch.cuda.synchronize()
    Matcher.raise_if_invalid()
    assert ENTRY not in launches and ops.FALLBACKS == fallbacks
