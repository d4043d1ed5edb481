"""CPU: the host half of tests/test_gpu_relation_head_edges.py.  (1) tests/relation_head_restated.py against the stand-in
``cpu_kernels.relation_head`` and against float64 autograd through it; (2) for EVERY grid case the GPU file launches, the claim
that makes a bitwise comparison legitimate: float32 evaluation equals float64, every operand and activation is a bf16 number,
gates are 0 / 0.5 / 1, both ReLU layers are mixed, nothing reaches 256, and the backward sums to the same bits in two fp32
orders ("the same bits" throughout: of the float64 result cast to float32, a zero of either sign being a zero -- ``bits``); (3) teeth: the bitwise assertion fails on six deliberately wrong compositions; (4) torch's own fp32 backward stays far
inside the derived bound that the real-valued GPU test applies."""
import pytest
import torch

import cpu_kernels
import relation_head_restated as RH

KEYS = ("duq", "duk", "dgate_q", "dgate_k", "dz")


def bits(x):
    """the bit patterns of a float32 tensor, -0.0 as +0.0.  The sign of a zero carries nothing here: the float64 reference keeps
    sigmoid(-200) = 1.4e-87 where fp32 has an exact 0, so a sum that is 0 in fp32 can be -1e-87 in float64 and casts to -0.0."""
    assert x.dtype == torch.float32
    return (x.contiguous() + 0.0).view(torch.int32)


def assert_forward_bits(got, want, what=""):
    """got / want: (rel, conn, gate_mean, h1, h2); gate_mean (index 2) is not a bitwise quantity.  Names the first mismatch."""
    for name, a, b in zip(("rel", "conn", None, "h1", "h2"), got, want):
        if name is None or a is None:
            continue
        b = b.float()
        assert a.shape == b.shape and a.dtype == torch.float32, (what, name, a.shape, b.shape)
        ne = bits(a) != bits(b)
        if bool(ne.any()):
            idx = tuple(int(x) for x in ne.nonzero()[0])
            raise AssertionError(f"{what}{name} differs in {int(ne.sum())} of {ne.numel()} elements, first at {idx}: "
                                 f"got {float(a[idx])!r}, want {float(b[idx])!r}")


def assert_backward_bits(got, want, what=""):
    for k in KEYS:
        a, b = got[k], want[k].float()
        ne = bits(a) != bits(b)
        if bool(ne.any()):
            idx = tuple(int(x) for x in ne.nonzero()[0])
            raise AssertionError(f"{what}{k} differs in {int(ne.sum())} of {ne.numel()} elements, first at {idx}: "
                                 f"got {float(a[idx])!r}, want {float(b[idx])!r}")


def _args(d, dtype):
    a = [d[n].to(dtype) for n in RH.NAMES]
    return a + [d["triplet"].to(dtype) if "triplet" in d else None, d.get("node_cls"), True]


# ---- 1. the restatement against the stand-in and against autograd -----------------------------------------------------------------
@pytest.mark.parametrize("B,N,T,R,C1", [(2, 6, 7, 50, 0), (1, 5, 3, 33, 9)])
def test_forward_restated_equals_the_stand_in_on_random_inputs(B, N, T, R, C1):
    d = RH.random_inputs(11 + N, B, N, T, R, C1)
    rel, conn, gm, h1, h2 = RH.forward(d)
    r2, c2, g2 = cpu_kernels.relation_head(*_args(d, torch.float64))
    assert rel.dtype == torch.float64 and tuple(h1.shape) == tuple(h2.shape) == (2, B * N * N, 256)
    for a, b in ((rel, r2), (conn, c2[..., 0]), (gm, g2)):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    # the saved activations are the ones the outputs were made from
    lin = torch.nn.functional.linear
    plain = RH.forward({k: v for k, v in d.items() if k not in ("triplet", "node_cls")})[0].reshape(-1, R)
    assert torch.allclose(lin(h2[0], d["w3r"].double(), d["b3r"].double()), plain, rtol=0, atol=1e-12)
    assert torch.allclose(lin(h2[1], d["w3c"].double(), d["b3c"].double())[:, 0], conn.reshape(-1), rtol=0, atol=1e-12)
    assert torch.allclose(torch.relu(lin(h1[0], d["w2r"].double(), d["b2r"].double())), h2[0], rtol=0, atol=1e-12)
    assert torch.allclose(torch.relu(lin(h1[1], d["w2c"].double(), d["b2c"].double())), h2[1], rtol=0, atol=1e-12)
    assert bool((h1 >= 0).all()) and bool((h2 >= 0).all())


@pytest.mark.parametrize("B,N,T", [(2, 5, 3), (1, 7, 7)])
def test_backward_pairs_restated_equals_float64_autograd(B, N, T, monkeypatch):
    """dh1 is taken from a hook on the pre-ReLU layer-1 value of the stand-in (the first relu it calls), dz from a hook on the
    gate logits (the argument of its sigmoid); the formulas then have to give autograd's gradients of the four inputs."""
    d = {k: v.double() for k, v in RH.random_inputs(3 + N, B, N, T, 20).items()}
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("gate_q", "gate_k", "uq", "uk")}
    seen = {}
    relu, sigmoid = torch.relu, torch.sigmoid

    def relu_hooked(x):
        if "dh1" not in seen and x.shape[-1] == 512:
            seen["dh1"] = None
            x.register_hook(lambda gr: seen.__setitem__("dh1", gr))
        return relu(x)

    def sigmoid_hooked(x):
        if "dz" not in seen:
            seen["dz"] = None
            x.register_hook(lambda gr: seen.__setitem__("dz", gr))
        return sigmoid(x)

    monkeypatch.setattr(torch, "relu", relu_hooked)
    monkeypatch.setattr(torch, "sigmoid", sigmoid_hooked)
    rel, conn, _ = cpu_kernels.relation_head(*[leaves.get(n, d[n]) for n in RH.NAMES])
    monkeypatch.undo()
    g = torch.Generator().manual_seed(5)
    loss = (rel * torch.randn(rel.shape, generator=g, dtype=torch.float64)).sum() + \
        (conn * torch.randn(conn.shape, generator=g, dtype=torch.float64)).sum()
    loss.backward()
    dh1 = seen["dh1"]                                                       # [B, N, N, 512]
    P = B * N * N
    dh1s = torch.stack([dh1[..., :256].reshape(P, 256), dh1[..., 256:].reshape(P, 256)], 0)
    out, mag = RH.backward_pairs(dh1s, d["gate_q"], d["gate_k"], d["uq"], d["uk"])
    want = dict(duq=leaves["uq"].grad, duk=leaves["uk"].grad, dgate_q=leaves["gate_q"].grad, dgate_k=leaves["gate_k"].grad,
                dz=seen["dz"])
    for k in KEYS:
        assert out[k].shape == want[k].shape and bool((mag[k] >= out[k].abs() * (1 - 1e-12)).all())
        assert float((out[k] - want[k]).abs().max()) <= 1e-12 * float(mag[k].max()), k
    loop = RH.backward_pairs(dh1s, d["gate_q"], d["gate_k"], d["uq"], d["uk"], order="loop", want_mag=False)[0]
    for k in KEYS:
        assert float((out[k] - loop[k]).abs().max()) <= 1e-12 * float(mag[k].max()), k


# ---- 2. the exactness claim, per grid case -------------------------------------------------------------------------------------------
def _bf16_exact(x):
    return torch.equal(x.bfloat16().to(x.dtype), x)


@pytest.mark.parametrize("case", RH.FORWARD_CASES, ids=RH.case_id)
def test_grid_forward_is_exact_in_float32_and_in_bf16(case):
    B, N, T, R, C1, sweep = case
    d = RH.grid_inputs(RH.case_seed(*case), B, N, T, R, C1, sweep)
    ref = RH.forward(d)
    f32 = RH.forward(d, dtype=torch.float32)
    for name, a, b in zip(("rel", "conn", "gate_mean", "h1", "h2"), f32, ref):
        if name != "gate_mean":   # a mean of 0 / 0.5 / 1 over B N N pairs: compared with the exact count below
            assert a.dtype == torch.float32 and torch.equal(a, b.float()), name      # float32 == float64 cast to float32
    assert_forward_bits(f32, ref)
    assert_forward_bits(RH.forward(d, dtype=torch.float32, round_bf16=True), ref, "h1, h2 through bf16: ")
    for k, v in d.items():
        if v.is_floating_point() and not k.startswith("gate_"):
            assert _bf16_exact(v), k                                                 # operands
    rel, conn, gm, h1, h2 = (x.float() for x in ref)
    for name, v in (("h1", h1), ("h2", h2), ("rel", rel), ("conn", conn)):
        assert _bf16_exact(v) and float(v.abs().max()) <= 256, (name, float(v.abs().max()))
    if C1:
        assert _bf16_exact(rel - d["triplet"][d["node_cls"][:, :, None], d["node_cls"][:, None, :]])
        assert int(d["node_cls"].min()) == 0 and int(d["node_cls"].max()) == C1 - 1
    g = RH.gates(d["gate_q"], d["gate_k"])                                            # fp32, as the kernels compute it
    assert torch.equal(g, RH.gates(d["gate_q"].double(), d["gate_k"].double()).float())
    assert bool(((g == 0) | (g == 0.5) | (g == 1)).all())
    assert float((ref[2] - RH.gate_mean_exact(d["gate_q"], d["gate_k"])).abs().max()) <= 1e-15
    if sweep:
        # every slot is the ONLY open slot of a pair of every image, and over the batch both of a subject-led pair (i, N - 1) and
        # of an object-led pair (N - 1, j)
        a, c = RH.sweep_slots(B, N, T)
        for b in range(B):
            for i in range(N - 1):
                assert torch.equal(g[b, i, N - 1], torch.nn.functional.one_hot(a[b, i], T).float())
                assert torch.equal(g[b, N - 1, i], torch.nn.functional.one_hot(c[b, i], T).float())
            assert set(a[b].tolist()) | set(c[b].tolist()) == set(range(T))
        assert set(a.flatten().tolist()) == set(c.flatten().tolist()) == set(range(T))
    else:
        for v in (0.0, 0.5, 1.0):
            assert float((g == v).float().mean()) >= 0.10, (v, float((g == v).float().mean()))
    for name, h in (("h1", h1), ("h2", h2)):
        on = float((h > 0).double().mean())
        assert 0.25 <= on <= 0.75, (name, on)


def test_grid_relation_logits_are_varied():
    """more than 100 distinct relation logits at the T sweep's shape: a kernel cannot pass by returning a constant"""
    case = (2, 9, 10, 33, 0, False)
    rel = RH.forward(RH.grid_inputs(RH.case_seed(*case), *case))[0]
    assert rel.unique().numel() > 100


@pytest.mark.parametrize("case", RH.BACKWARD_CASES, ids=RH.case_id)
def test_grid_backward_is_exact_in_float32_in_two_summation_orders(case):
    B, N, T = case
    d = RH.grid_inputs(RH.case_seed(*case), B, N, T, 1)
    dh1 = RH.grid_dh1(RH.case_seed(*case) + 1, B, N)
    a = (dh1, d["gate_q"], d["gate_k"], d["uq"], d["uk"])
    ref = RH.backward_pairs(*a, want_mag=False)[0]
    for order in ("einsum", "loop"):
        got = RH.backward_pairs(*a, dtype=torch.float32, order=order, want_mag=False)[0]
        for k in KEYS:
            assert torch.equal(got[k], ref[k].float()), (order, k)
        assert_backward_bits(got, ref, order + ": ")
    assert float(ref["dz"].abs().max()) > 0 and float(ref["duq"].abs().max()) > 0
    assert torch.equal(ref["dz"].float() * 4, (ref["dz"].float() * 4).round())     # dz = integer x 0.25 (g = 0.5) or 0


# ---- 3. teeth ---------------------------------------------------------------------------------------------------------------------------
def _f32(t):
    return tuple(None if x is None else x.float() for x in t)


@pytest.mark.parametrize("what,case,wrong", [
    ("slot T - 1 dropped", (2, 9, 1, 33, 0, False), dict(drop_slot=0)),
    ("slot T - 1 dropped", (2, 9, 10, 33, 0, True), dict(drop_slot=9)),
    ("i and j swapped in the uk lookup", (3, 3, 7, 50, 12, False), dict(swap_uk=True)),
    ("last ragged object column unwritten", (3, 1, 7, 50, 12, False), dict(skip_last_col=True)),
    ("frequency bias indexed [cls_j, cls_i]", (3, 3, 7, 50, 12, False), dict(swap_bias=True)),
])
def test_forward_bit_assertion_fails_on_a_wrong_composition(what, case, wrong):
    """the smallest listed case where the defect applies (N = 1 has no second query to swap with, but its only object column is
    already a ragged one in every tiling)"""
    assert case in RH.FORWARD_CASES
    d = RH.grid_inputs(RH.case_seed(*case), *case)
    ref = RH.forward(d)
    assert_forward_bits(_f32(RH.forward(d, dtype=torch.float32)), ref)
    with pytest.raises(AssertionError, match="differs in"):
        assert_forward_bits(_f32(RH.forward(d, dtype=torch.float32, **wrong)), ref)
    if "drop_slot" in wrong:   # the logits alone notice
        with pytest.raises(AssertionError, match="rel differs in"):
            assert_forward_bits(_f32(RH.forward(d, dtype=torch.float32, **wrong))[:2], ref[:2])


@pytest.mark.parametrize("what,case,wrong", [
    ("m >= 256 skipped", (1, 257, 2), dict(skip_from=256)),
    ("uk half of dg omitted", (2, 1, 7), dict(omit_uk=True)),
])
def test_backward_bit_assertion_fails_on_a_wrong_composition(what, case, wrong):
    assert case in RH.BACKWARD_CASES
    B, N, T = case
    d = RH.grid_inputs(RH.case_seed(*case), B, N, T, 1)
    dh1 = RH.grid_dh1(RH.case_seed(*case) + 1, B, N)
    a = (dh1, d["gate_q"], d["gate_k"], d["uq"], d["uk"])
    ref = RH.backward_pairs(*a, want_mag=False)[0]
    assert_backward_bits(RH.backward_pairs(*a, dtype=torch.float32, want_mag=False)[0], ref)
    with pytest.raises(AssertionError, match="differs in"):
        assert_backward_bits(RH.backward_pairs(*a, dtype=torch.float32, want_mag=False, **wrong)[0], ref)
    # N = 256 has no m >= 256: the defect does not apply one step below
    if "skip_from" in wrong:
        c2 = (1, 256, 2)
        d = RH.grid_inputs(RH.case_seed(*c2), 1, 256, 2, 1)
        a = (RH.grid_dh1(RH.case_seed(*c2) + 1, 1, 256), d["gate_q"], d["gate_k"], d["uq"], d["uk"])
        assert_backward_bits(RH.backward_pairs(*a, dtype=torch.float32, want_mag=False, **wrong)[0],
                             RH.backward_pairs(*a, want_mag=False)[0])


# ---- 4. the derived bound of the real-valued backward test --------------------------------------------------------------------------
def real_backward_inputs(B, N, T):
    g = torch.Generator().manual_seed(77 + N + T)
    d = RH.random_inputs(78 + N + T, B, N, T, 1)
    return (torch.randn(2, B * N * N, 256, generator=g), d["gate_q"], d["gate_k"], d["uq"], d["uk"])


@pytest.mark.parametrize("case", RH.BACKWARD_REAL, ids=RH.case_id)
def test_torch_fp32_backward_is_far_inside_the_derived_bound(case):
    B, N, T = case
    a = real_backward_inputs(B, N, T)
    ref, mag = RH.backward_pairs(*a)
    bound = RH.backward_bound(mag, N)
    got = RH.backward_pairs(*a, dtype=torch.float32, want_mag=False)[0]
    for k in KEYS:
        ratio = float(((got[k].double() - ref[k]).abs() / bound[k]).max())
        print(f"{RH.case_id(case)} {k}: torch fp32 |err| / bound = {ratio:.4f}")
        assert ratio <= 0.25, (k, ratio)
