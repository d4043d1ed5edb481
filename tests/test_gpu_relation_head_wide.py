"""GPU (-m gpu): the relation head above 64 predicate classes -- egtr_rel_head_forward_wide_f32 ("wide_f32", with and without
the save buffers), egtr_rel_head_forward_wide_bf16x6_f32 on the streams of egtr_rel_head_streams_wide_f32 ("wide_x6").  The host
half, tests/test_relation_head_wide_cases_cpu.py, proves per case that the grid inputs make a bitwise comparison legitimate and
that they tell the 32-wide output tiles apart.

Every output is the front of a NaN-filled buffer with a NaN guard band behind it: a pair a kernel never writes shows, and so
does a store past the end of an output.

  * grid, bitwise against the float64 restatement: R = 33 .. 256 on both sides of every 32- and 64-column boundary, N = 1 .. 33
    at R = 100 with the frequency bias, every slot count at R = 97; the sigmoid epilogue of the x6 entry;
  * the same bits as the narrow sibling where both serve (R = 33, 64);
  * real-valued inputs against float64 (the 2e-4 / 1e-5 of test_gpu_pinning.py::test_relation_head_kernels_vs_oracle_reference_order)
    and, per 64-column block, against the narrow sibling run on that block's slices of W3 / b3 / frequency table under a
    derived rounding bound;
  * containment of a non-finite table entry, refusals, and training through ops.relation_head under every mode."""
import functools
import math

import pytest
import torch

import relation_head_restated as RH
from test_relation_head_cases_cpu import bits
from test_relation_head_wide_cases_cpu import WIDE_N_SWEEP, WIDE_R_SWEEP, WIDE_T_SWEEP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
GUARD = 1024   # floats behind each output
WIDE = ("wide_f32", "wide_f32_nosave", "wide_x6")


def _entries(T):
    return [e for e in WIDE if not (e == "wide_x6" and T > 9)]


def _guarded(shape):
    n = math.prod(shape)
    buf = torch.full((n + GUARD,), NAN, device=DEV)
    return buf[:n].view(shape), buf


def _launch(entry, d, declare=None, node_cls="given", into=None, sigmoid=False):
    """One wide entry on the tensors of ``d`` (device, float32).  Returns dict(rel, conn, gm, h1, h2, guards); h1 / h2 None where
    no save buffer is passed.  ``declare`` / ``into`` as in test_gpu_relation_head_edges.py."""
    from egtr_amd import _lib, ops
    B, N, T = d["gate_q"].shape
    R = d["w3r"].shape[0]
    P = B * N * N
    n = dict(T=T, R=R, hidden=256)
    n.update(declare or {})
    out, guards = dict(h1=None, h2=None), []
    for k, shape in (("rel", (B, N, N, R)), ("conn", (B, N, N))) + ((("h1", (2, P, 256)), ("h2", (2, P, 256)))
                                                                    if entry == "wide_f32" else ()):
        out[k], buf = _guarded(shape)
        guards.append(buf)
    gmbuf = torch.zeros(T + GUARD, device=DEV)
    out["gm"], out["guards"], out["gmbuf"] = gmbuf[:T], guards, gmbuf
    if into is not None:
        into.update(out)
    trip = d.get("triplet")
    ncls = d.get("node_cls") if node_cls == "given" else None
    tail = [_lib.ptr(trip), _lib.ptr(ncls), B, N, n["T"], n["hidden"], n["R"], 0 if trip is None else trip.shape[0],
            out["rel"].data_ptr(), out["conn"].data_ptr(), out["gm"].data_ptr()]

    def p(*names):
        return [d[k].data_ptr() for k in names]

    if entry in ("wide_f32", "wide_f32_nosave"):
        _lib.launch("egtr_rel_head_forward_wide_f32", *p(*RH.NAMES), *tail, _lib.ptr(out["h1"]), _lib.ptr(out["h2"]))
    else:
        w2xr, w3x, w2xc = ops.rel_head_streams_wide(d["w2r"], d["w3r"][:256], d["w2c"])
        args = p("gate_q", "gate_k", "uq", "uk", "b1") + [w2xr.data_ptr()] + p("b2r") + [w3x.data_ptr()] + p("b3r") + \
            [w2xc.data_ptr()] + p("b2c", "w3c", "b3c") + tail
        _lib.launch("egtr_rel_head_forward_wide_bf16x6_f32", *args, 1 if sigmoid else 0)
    torch.cuda.synchronize()
    return out


def _check_guards(entry, out, T, what=""):
    n_out = [out[k].numel() for k in ("rel", "conn", "h1", "h2") if out[k] is not None]
    for buf, n in zip(out["guards"], n_out):
        assert bool(torch.isnan(buf[n:]).all()), f"{what}{entry}: wrote behind an output of {n} floats"
    assert bool((out["gmbuf"][T:] == 0).all()), f"{what}{entry}: wrote behind gate_mean"


def _check_bits(entry, out, ref, what=""):
    B, N = out["conn"].shape[:2]
    for name in ("rel", "conn", "h1", "h2"):
        a, want = out[name], ref[name]
        if a is None:
            continue
        assert a.shape == want.shape and a.dtype == torch.float32
        ne = bits(a) != bits(want)
        if bool(ne.any()):
            idx = [int(x) for x in ne.nonzero()[0]]
            if name in ("h1", "h2"):
                b, i, j, tag = idx[1] // (N * N), idx[1] // N % N, idx[1] % N, f"mlp {idx[0]}, channel {idx[2]}"
            else:
                b, i, j, tag = idx[0], idx[1], idx[2], (f"relation {idx[3]} (output tile {idx[3] // 32})" if name == "rel"
                                                        else "connectivity")
            raise AssertionError(f"{what}{entry}: {name} differs in {int(ne.sum())} of {ne.numel()} elements, first at (b {b}, i {i}, "
                                 f"j {j}), {tag}: got {float(a[tuple(idx)])!r}, want {float(want[tuple(idx)])!r}; 8 x 4 tile "
                                 f"(i0 {i // 8 * 8}, j0 {j // 4 * 4}), lanes {(i % 8) * 4 + j % 4} and +32")


def _check_gate_mean(entry, gm, want, B, N):
    """the bound test_gpu_relation_head_edges.py derives: one fp32 atomic add per 8 x 4 tile, (adds + 2) ulps of the result"""
    adds = B * ((N + 7) // 8) * ((N + 3) // 4)
    for t, (g, w) in enumerate(zip(gm.cpu().double().tolist(), want.tolist())):
        bound = (adds + 2) * 2.0 ** (math.floor(math.log2(w)) - 23) if w > 0 else 0.0
        assert abs(g - w) <= bound, f"{entry}: gate_mean[{t}] = {g!r}, exact {w!r}, |diff| {abs(g - w):.3e} > {bound:.3e} ({adds} adds)"


@functools.lru_cache(maxsize=4)
def _case(case):
    """(inputs on the device, float64 reference cast to float32 with the float64 logits, exact gate means); never written to"""
    B, N, T, R, C1, sweep = case
    d = RH.grid_inputs(RH.case_seed(*case), B, N, T, R, C1, sweep)
    gm = RH.gate_mean_exact(d["gate_q"], d["gate_k"])
    d = {k: v.to(DEV) for k, v in d.items()}
    rel, conn, _, h1, h2 = RH.forward(d)
    assert rel.dtype == torch.float64
    return d, dict(rel=rel.float(), conn=conn.float(), h1=h1.float(), h2=h2.float(), rel64=rel, conn64=conn), gm


def _run_case(case, entries):
    B, N, T = case[:3]
    d, ref, gm = _case(case)
    for entry in entries:
        out = _launch(entry, d)
        _check_bits(entry, out, ref, RH.case_id(case) + " ")
        _check_guards(entry, out, T, RH.case_id(case) + " ")
        _check_gate_mean(entry, out["gm"], gm, B, N)


# ---- 1. grid inputs, bitwise ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WIDE_R_SWEEP, ids=RH.case_id)
def test_wide_every_relation_count_edge_is_bitwise_the_float64_restatement(case):
    """(2, 9, 7, R), without and with the frequency bias: R on both sides of every 32-column (output tile) and 64-column boundary up
    to 256, and 33 / 64 where the narrow entries serve too"""
    _run_case(case, _entries(7))


@pytest.mark.parametrize("case", WIDE_N_SWEEP, ids=RH.case_id)
def test_wide_every_query_count_edge_is_bitwise_the_float64_restatement(case):
    """R = 100 (four output tiles, the last ragged), T = 7, frequency bias with classes 0 and C1 - 1: N = 1, N < 4, whole and ragged
    8 x 4 tiles, more than one tile row"""
    _run_case(case, _entries(7))


@pytest.mark.parametrize("case", WIDE_T_SWEEP, ids=RH.case_id)
def test_wide_every_slot_count_is_bitwise_the_float64_restatement(case):
    """(2, 9, T, 97) for every served T (x6: 1 .. 9) and the slot-sweep gates at T = 7, 9, 10"""
    _run_case(case, _entries(case[2]))


@pytest.mark.parametrize("case", [WIDE_R_SWEEP[5], WIDE_R_SWEEP[-1]], ids=RH.case_id)
def test_wide_x6_sigmoid_epilogue_is_the_sigmoid_of_its_logits(case):
    """apply_sigmoid = 1 on the grid (the logits are the float64 values exactly): sigmoid in float64, to 1 ulp of fp32"""
    d, ref, _ = _case(case)
    out = _launch("wide_x6", d, sigmoid=True)
    _check_guards("wide_x6", out, case[2])
    for name in ("rel", "conn"):
        want = torch.sigmoid(ref[name + "64"])
        ulp = torch.pow(2.0, torch.floor(torch.log2(want.clamp_min(2.0 ** -126))) - 23)
        err = (out[name].double() - want).abs()
        assert bool((err <= ulp).all()), (name, float((err / ulp).max()))


@pytest.mark.parametrize("case", [c for c in WIDE_R_SWEEP if c[3] in (33, 64)], ids=RH.case_id)
def test_wide_entries_return_the_bits_of_their_narrow_siblings_where_both_serve(case):
    import test_gpu_relation_head_edges as narrow
    d, _, _ = _case(case)
    for wide, sib in (("wide_f32", "f32"), ("wide_x6", "x6")):
        a, b = _launch(wide, d), narrow._launch(sib, d)
        for name in ("rel", "conn", "h1", "h2"):
            if a[name] is not None:
                assert torch.equal(bits(a[name]), bits(b[name])), (wide, name)
        assert float((a["gm"] - b["gm"]).abs().max()) <= 1e-6   # atomics in either: equal to their rounding


# ---- 2. real-valued inputs ----------------------------------------------------------------------------------------------------------
REAL = [(2, 40, 7, 100), (1, 65, 4, 200)]


@functools.lru_cache(maxsize=2)
def _real(case):
    B, N, T, R = case
    d = RH.random_inputs(RH.case_seed(*case), B, N, T, R, 6)
    d = {k: v.to(DEV) for k, v in d.items()}
    rel, conn, gm, h1, h2 = RH.forward(d)
    return d, dict(rel=rel, conn=conn, gm=gm, h2=h2)


@pytest.mark.parametrize("case", REAL, ids=RH.case_id)
def test_wide_entries_real_valued_vs_float64_and_vs_the_narrow_sibling_per_column_block(case):
    """Standard-normal inputs, frequency bias on.
    (a) Each wide entry against the float64 restatement: 2e-4 on both logits, 1e-5 on the gate means (the tolerances of
        test_gpu_pinning.py::test_relation_head_kernels_vs_oracle_reference_order).
    (b) Columns [64 g, 64 g + 64) against the narrow sibling launched on rows 64 g .. of W3 / b3 and the same columns of the
        frequency table: |wide - narrow| <= 2 (256 + 8) 2^-24 sum_k |w3[r, k] h2[k]| per element, h2 from float64.  Layers 1 and 2
        are the sibling's instruction for instruction (asserted bitwise on the saved h1 / h2 of the f32 pair), so the two differ
        only in the fp32 additions of layer 3: each sums 256 products (exact f32 entry: fp32 products, one rounding each, inside
        the 8) and adds b3 and the frequency bias, at most 256 + 8 roundings each of at most 2^-24 of the running sum of absolute
        values.  The x6 pair needs no other constant: its products are exact, its main chain is 16 (wide) or 8
        (narrow, per wave) accumulations, the five correction terms are below 2^-7 of the main one and the three dropped ones
        below 3 x 2^-24 of it -- all inside the 256 + 8 that the fp32 chain needs.
    Largest |wide - narrow| / bound measured on the MI355X: 0.0118 (exact f32 pair, (1, 65, 4, 200)) and 0.0093 at (2, 40, 7, 100);
    the x6 pair 0.0073 and 0.0068.  Against float64: rel <= 3.2e-6, conn <= 1.2e-6, gate means <= 1.3e-7.  conn, h1 and h2 are
    bitwise the sibling's."""
    import test_gpu_relation_head_edges as narrow
    B, N, T, R = case
    d, ref = _real(case)
    outs = {e: _launch(e, d) for e in ("wide_f32", "wide_x6")}
    for e, out in outs.items():
        _check_guards(e, out, T)
        err_rel = float((out["rel"].double() - ref["rel"]).abs().max())
        err_conn = float((out["conn"].double() - ref["conn"]).abs().max())
        err_gm = float((out["gm"].double() - ref["gm"]).abs().max())
        print(f"{RH.case_id(case)} {e}: max |rel - f64| = {err_rel:.3e}, |conn - f64| = {err_conn:.3e}, |gm - f64| = {err_gm:.3e}")
        assert err_rel < 2e-4 and err_conn < 2e-4 and err_gm < 1e-5, (e, err_rel, err_conn, err_gm)
    mag = ref["h2"][0].abs() @ d["w3r"].double().abs().t()                      # [B N N, R]
    bound = (2 * (256 + 8) * 2.0 ** -24 * mag).view(B, N, N, R)
    worst = {}
    for wide, sib in (("wide_f32", "f32"), ("wide_x6", "x6")):
        worst[wide] = 0.0
        for g in range((R + 63) // 64):
            sl = slice(64 * g, min(64 * g + 64, R))
            x = dict(d, w3r=d["w3r"][sl].contiguous(), b3r=d["b3r"][sl].contiguous(), triplet=d["triplet"][..., sl].contiguous())
            nb = narrow._launch(sib, x)
            diff = (outs[wide]["rel"][..., sl].double() - nb["rel"].double()).abs()
            worst[wide] = max(worst[wide], float((diff / bound[..., sl]).max()))
            assert torch.equal(bits(outs[wide]["conn"]), bits(nb["conn"])), (wide, g)
            if nb["h1"] is not None:
                assert torch.equal(bits(outs[wide]["h1"]), bits(nb["h1"])) and torch.equal(bits(outs[wide]["h2"]), bits(nb["h2"]))
        print(f"{RH.case_id(case)} {wide} vs {sib} per 64-column block: max |diff| / bound = {worst[wide]:.5f}")
    assert max(worst.values()) <= 1.0, worst


# ---- 3. containment of non-finite table entries -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _real_small():
    d = RH.random_inputs(4243, 2, 13, 7, 100)
    return {k: v.to(DEV) for k, v in d.items()}


@pytest.mark.parametrize("entry", WIDE)
@pytest.mark.parametrize("table,at,value", [("uq", (1, 5, 2), NAN), ("uk", (0, 9, 6), float("inf"))], ids=["nan_uq", "inf_uk"])
def test_wide_a_non_finite_table_entry_stays_in_its_row_or_column(entry, table, at, value):
    """(2, 13, 7, 100): one channel of uq[1, 5, 2] = NaN / of uk[0, 9, 6] = +inf, once per MLP half: every pair of that subject row
    (object column) is non-finite in ALL 100 columns of that MLP's output, every other element keeps the bits of the clean launch"""
    d = _real_small()
    clean = _launch(entry, d)
    assert bool(torch.isfinite(clean["rel"]).all()) and bool(torch.isfinite(clean["conn"]).all())
    b, q, t = at
    for half, (hit, other) in enumerate((("rel", "conn"), ("conn", "rel"))):
        x = dict(d)
        x[table] = d[table].clone()
        x[table][b, q, t, 256 * half + 77] = value
        out = _launch(entry, x)
        mask = torch.zeros(2, 13, 13, dtype=torch.bool, device=DEV)
        if table == "uq":
            mask[b, q, :] = True
        else:
            mask[b, :, q] = True
        got = out[hit].reshape(2, 13, 13, -1)
        assert not bool(torch.isfinite(got)[mask].any()), f"{entry}: finite {hit} output inside row / column {q}"
        same = (bits(got) == bits(clean[hit].reshape(2, 13, 13, -1))).all(-1)
        spilled = (~same & ~mask).nonzero().tolist()
        assert not spilled, f"{entry}: {hit} changed outside row / column {q} at (b, i, j) = {spilled[:12]} ({len(spilled)} pairs)"
        assert torch.equal(bits(out[other]), bits(clean[other])), f"{entry}: {other} changed by a {hit}-half channel"


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", WIDE)
def test_wide_entries_refuse_what_they_do_not_serve(entry):
    """num_rel = 257, a slot count past the entry's range, hidden = 128: status -3, nothing written"""
    from egtr_amd import _lib
    bad_T = 10 if entry == "wide_x6" else 11
    for T, R, declare in [(7, 257, None), (bad_T, 100, None), (7, 100, dict(hidden=128))]:
        d = {k: v.to(DEV) for k, v in RH.random_inputs(5, 1, 5, T, R).items()}
        out = {}
        with pytest.raises(_lib.EgtrHipError, match=r"status -3"):
            _launch(entry, d, declare=declare, into=out)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(buf).all()) for buf in out["guards"]) and bool((out["gmbuf"] == 0).all()), (entry, T, R, declare)
    d = {k: v.to(DEV) for k, v in RH.random_inputs(7, 1, 5, 7, 100, 6).items()}
    with pytest.raises(_lib.EgtrHipError, match=r"status -1"):
        _launch(entry, d, node_cls=None)


def test_more_than_256_predicates_stay_an_error_of_the_binding():
    from egtr_amd import _lib, ops
    d = {k: v.to(DEV) for k, v in RH.random_inputs(8, 1, 5, 7, 257).items()}
    with pytest.raises(_lib.EgtrHipError, match=r"status -3"):
        ops.relation_head(*[d[k] for k in RH.NAMES])
    with pytest.raises(_lib.EgtrHipError, match=r"status -3"):
        ops.rel_head_streams_wide(d["w2r"], d["w3r"], d["w2c"])


# ---- 5. the routes of ops.relation_head --------------------------------------------------------------------------------------------
def test_relation_head_routes_above_64_predicates(monkeypatch):
    """inference with an owner: the wide x6 entry, streams cached under a key of their own; bf16 inputs: the fp32 wide kernel on
    widened operands, cast back, and neither bf16 entry is called"""
    from egtr_amd import _lib, ops
    d, ref = _real(REAL[0])
    names = []
    real_launch = _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda name, *a, **k: (names.append(name), real_launch(name, *a, **k))[1])
    owner = torch.nn.Module()
    before = dict(ops.FALLBACKS)
    with torch.no_grad():
        rel, conn, gm = ops.relation_head(*[d[k] for k in RH.NAMES], d["triplet"], d["node_cls"], True, owner=owner)
        rel2, _, _ = ops.relation_head(*[d[k] for k in RH.NAMES], d["triplet"], d["node_cls"], True, owner=owner)
    assert names == ["egtr_rel_head_streams_wide_f32", "egtr_rel_head_forward_wide_bf16x6_f32", "egtr_rel_head_forward_wide_bf16x6_f32"]
    assert torch.equal(rel, rel2) and float((rel.double() - ref["rel"]).abs().max()) < 2e-4
    assert float((conn[..., 0].double() - ref["conn"]).abs().max()) < 2e-4
    del names[:]
    with torch.no_grad():
        relb, connb, _ = ops.relation_head(*[d[k].bfloat16() for k in RH.NAMES], d["triplet"], d["node_cls"], False)
    assert names == ["egtr_rel_head_forward_wide_f32"] and relb.dtype == connb.dtype == torch.bfloat16
    with pytest.raises(ValueError):
        ops.relation_head_bf16w(*[d[k].bfloat16() for k in RH.NAMES])
    assert ops.FALLBACKS == before


def _grads(d, trip, node, g_rel, g_conn):
    from egtr_amd import ops
    leaves = {k: d[k].clone().requires_grad_(True) for k in RH.NAMES}
    rel, conn, gm = ops.relation_head(*leaves.values(), trip, node, True)
    ((rel * g_rel).sum() + (conn[..., 0] * g_conn).sum()).backward()
    return rel.detach(), conn.detach(), gm, {k: v.grad for k, v in leaves.items()}


def test_training_through_relation_head_at_100_predicates_under_every_mode(monkeypatch):
    """(2, 9, 7, 100) with requires_grad: every gradient of RelationHeadFunction against autograd through the float64 restatement
    (1e-3 of the largest gradient, the tolerance of test_gpu_kernels.py::test_relation_head_backward_matches_autograd for
    B N N <= 4096; logits 2e-4).  Matmul precision "bf16" and the deterministic mode take the same exact-f32 entry (the same logits
    bit for bit); under the deterministic mode two runs give the same bits; nothing is counted in FALLBACKS."""
    from egtr_amd import _lib, ops
    B, N, T, R = 2, 9, 7, 100
    d = {k: v.to(DEV) for k, v in RH.random_inputs(77, B, N, T, R, 6).items()}
    trip, node = d["triplet"], d["node_cls"]
    g = torch.Generator().manual_seed(78)
    g_rel, g_conn = torch.randn(B, N, N, R, generator=g).to(DEV), torch.randn(B, N, N, generator=g).to(DEV)
    d64 = {k: d[k].double().requires_grad_(True) for k in RH.NAMES}
    rrel, rconn, rgm, _, _ = RH.forward(dict(d64, triplet=trip, node_cls=node))
    ((rrel * g_rel.double()).sum() + (rconn * g_conn.double()).sum()).backward()
    names = []
    real_launch = _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda name, *a, **k: (names.append(name), real_launch(name, *a, **k))[1])
    before = dict(ops.FALLBACKS)

    def check(run):
        rel, conn, gm, grads = run
        assert float((rel.double() - rrel.detach()).abs().max()) < 2e-4 and float((conn[..., 0].double() - rconn.detach()).abs().max()) < 2e-4
        assert float((gm.double() - rgm.detach()).abs().max()) < 1e-5
        for k in RH.NAMES:
            want = d64[k].grad
            err = float((grads[k].double() - want).abs().max())
            assert err < 1e-3 * max(1.0, float(want.abs().max())), (k, err)

    base = _grads(d, trip, node, g_rel, g_conn)
    check(base)
    assert names.count("egtr_rel_head_forward_wide_f32") == 1 and not any("bf16" in n and "rel_head" in n for n in names)
    with ops.matmul_precision_mode("bf16"):
        del names[:]
        low = _grads(d, trip, node, g_rel, g_conn)
        assert names.count("egtr_rel_head_forward_wide_f32") == 1 and not any("bf16" in n and "rel_head" in n for n in names)
    check(low)
    assert torch.equal(low[0], base[0]) and torch.equal(low[1], base[1])
    with ops.deterministic():
        del names[:]
        det1 = _grads(d, trip, node, g_rel, g_conn)
        det2 = _grads(d, trip, node, g_rel, g_conn)
        assert names.count("egtr_rel_head_forward_wide_f32") == 2
    check(det1)
    assert torch.equal(det1[0], base[0]) and torch.equal(det1[1], base[1])
    assert torch.equal(det1[2], det2[2]) and all(torch.equal(det1[3][k], det2[3][k]) for k in RH.NAMES)
    assert ops.FALLBACKS == before
