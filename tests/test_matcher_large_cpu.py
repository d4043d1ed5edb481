"""CPU: the public surface of the device matcher for proposal-sized query sets (egtr_hungarian_match_large_f32, the
two-stage variant's per-token proposals) that needs no GPU -- the workspace query, the argument checks that come before any
HIP call, the routing predicate shared by ``ops.hungarian_match`` and ``DeformableDetrHungarianMatcher.prepare``, and the
restated solver (oracle/lsa.py) against scipy on the tied matrices the GPU tests solve."""
import ctypes

import numpy as np
import pytest

import matcher_large_cases as MC
from oracle import lsa

E_ARG, E_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def h():
    from egtr_amd import _lib
    return _lib.lib()


def test_workspace_query_grows_with_batch_queries_and_targets(h):
    q = h.egtr_hungarian_match_large_workspace_bytes
    base = q(4, 12537, 30, 100)
    assert base > 0
    assert q(5, 12537, 30, 100) > base
    assert q(4, 12538, 30, 100) > base
    assert q(4, 12537, 30, 101) > base
    # the fp32 cost blocks of the whole batch and the 36 bytes of solver state per column have to fit
    assert base >= 4 * 12537 * 100 + 4 * 36 * 12537
    assert q(16, 22223, 100, 1600) >= 4 * 22223 * 1600 + 16 * 36 * 22223
    assert q(1, 65536, 512, 512) > 0 and q(1, 2, 1, 1) > 0 and q(1, 65, 1, 1) > 0


@pytest.mark.parametrize("batch,N,T,total", [
    (1, 30, 30, 30), (1, 30, 31, 31), (2, 1500, 1500, 1600),       # T >= N: not the transposed problem
    (1, 2000, 513, 513), (4, 65536, 600, 2000),                    # T > 512
    (1, 65537, 30, 30), (2, 100000, 512, 600),                     # N > 65 536
    (0, 1500, 30, 30), (1, 0, 0, 0), (1, 1500, -1, 0),             # nothing to solve
])
def test_workspace_query_is_zero_outside_the_domain(h, batch, N, T, total):
    assert h.egtr_hungarian_match_large_workspace_bytes(batch, N, T, total) == 0


def _host_words(n=64):
    """A host buffer and its address: the checks under test return before anything dereferences a pointer."""
    buf = ctypes.create_string_buffer(n + 16)
    return buf, (ctypes.addressof(buf) + 15) & ~15


def _call(h, p, batch=2, N=1500, K=1, T=30, cost_in=None, workspace=None, workspace_bytes=0, **null):
    a = dict(logits=p, boxes=p, tgt_ids=p, tgt_boxes=p, tgt_offsets=p, out_offsets=p, pred_idx=p, tgt_idx=p, match_cost=p)
    a.update(null)
    return h.egtr_hungarian_match_large_f32(None, a["logits"], a["boxes"], a["tgt_ids"], a["tgt_boxes"], a["tgt_offsets"],
                                            a["out_offsets"], batch, N, K, T, 1.0, 5.0, 2.0, 0, 0.0, 0.0, a["pred_idx"],
                                            a["tgt_idx"], a["match_cost"], None, cost_in, None, workspace, workspace_bytes)


def test_null_pointers_and_small_workspaces_are_rejected_without_a_gpu(h):
    buf, p = _host_words()
    need = h.egtr_hungarian_match_large_workspace_bytes(2, 1500, 30, 30)   # the least a batch with max_targets 30 needs
    assert need > 0
    for name in ("tgt_offsets", "out_offsets", "pred_idx", "tgt_idx", "match_cost"):
        assert _call(h, p, workspace=p, workspace_bytes=need, **{name: None}) == E_ARG, name
        assert _call(h, p, cost_in=p, workspace=p, workspace_bytes=need, **{name: None}) == E_ARG, name
    for name in ("logits", "boxes", "tgt_ids", "tgt_boxes"):               # required unless a matrix is given
        assert _call(h, p, workspace=p, workspace_bytes=need, **{name: None}) == E_ARG, name
    assert _call(h, p, batch=0, workspace=p, workspace_bytes=need) == E_ARG
    assert _call(h, p, K=0, workspace=p, workspace_bytes=need) == E_ARG
    assert _call(h, p, workspace=None, workspace_bytes=need) == E_ARG
    assert _call(h, p, workspace=p, workspace_bytes=need - 1) == E_ARG
    assert _call(h, p, workspace=p, workspace_bytes=0) == E_ARG
    assert _call(h, p, cost_in=p, workspace=p, workspace_bytes=-5) == E_ARG
    # an image-free problem is served without a launch (and without a workspace), like the one-wave entry
    assert _call(h, p, T=0) == 0
    from egtr_amd import _lib
    with pytest.raises(_lib.EgtrHipError):
        _lib.check(E_ARG, "x")


@pytest.mark.parametrize("N,T", [(30, 30), (30, 40), (1500, 1500), (2000, 513), (65537, 30), (100000, 600)])
def test_shapes_outside_the_domain_are_unsupported_without_a_gpu(h, N, T):
    buf, p = _host_words()
    assert _call(h, p, N=N, T=T, workspace=p, workspace_bytes=1 << 40) == E_UNSUPPORTED
    assert _call(h, p, N=N, T=T, cost_in=p, workspace=p, workspace_bytes=1 << 40) == E_UNSUPPORTED


def test_the_one_wave_entry_keeps_its_limit(h):
    buf, p = _host_words()
    st = h.egtr_hungarian_match_f32(None, p, p, p, p, p, p, 2, 1500, 1, 30, 1.0, 5.0, 2.0, 0, 0.0, 0.0, p, p, p, None, None,
                                    None, None)
    assert st == E_UNSUPPORTED
    assert h.egtr_abi_version() == 7


def test_routing_predicate_on_both_sides_of_every_bound():
    from egtr_amd import ops
    route = ops.hungarian_match_route
    # up to 1024 a side: the one-wave kernel, as before (wide problems included)
    for N, T in ((200, 30), (200, 0), (1024, 1024), (1024, 1), (37, 300), (100, 1024), (1, 1)):
        assert route(N, T) == "small", (N, T)
    # N beyond 1024: the 16-wave kernel inside T < N, T <= 512, N <= 65 536
    for N, T in ((1025, 0), (1025, 1), (1025, 512), (1500, 12), (12537, 40), (22223, 100), (65536, 512), (65536, 1)):
        assert route(N, T) == "large", (N, T)
    # everything else: the host route
    for N, T in ((1025, 513), (1025, 1025), (1025, 1100), (65537, 1), (65537, 512), (100000, 30), (200, 1025), (1024, 1025),
                 (600, 2000), (12537, 513)):
        assert route(N, T) is None, (N, T)
    assert (ops.HUNGARIAN_MAX_SIDE, ops.HUNGARIAN_LARGE_MAX_TARGETS, ops.HUNGARIAN_LARGE_MAX_QUERIES) == (1024, 512, 65536)


def test_route_agrees_with_the_workspace_query(h):
    """Wherever the predicate says "large", the C entry's own domain check (the workspace query) agrees."""
    from egtr_amd import ops
    for N in (1, 2, 1024, 1025, 1500, 65536, 65537):
        for T in (0, 1, 511, 512, 513, 1024, 1025, N - 1, N):
            if T < 0:
                continue
            in_domain = h.egtr_hungarian_match_large_workspace_bytes(1, N, T, max(T, 1)) > 0
            assert in_domain == (T < N and T <= 512 and N <= 65536), (N, T)
            if ops.hungarian_match_route(N, T) == "large":
                assert in_domain, (N, T)


@pytest.mark.parametrize("build", [c[1] for c in MC.DUPLICATED_CASES + MC.TIE_CASES],
                         ids=[c[0] for c in MC.DUPLICATED_CASES + MC.TIE_CASES])
def test_restated_solver_equals_scipy_on_the_tied_matrices(build):
    """oracle/lsa.py (the algorithm csrc/matcher.hip restates) returns scipy's indices on the tied matrices of the GPU tests:
    tied integer costs, the lower half of the rows duplicated, an all-equal matrix, identical padded queries."""
    from scipy.optimize import linear_sum_assignment as sp
    c = build()
    a, b = sp(c)
    ra, rb = lsa.linear_sum_assignment(c)
    assert np.array_equal(a, ra) and np.array_equal(b, rb)
