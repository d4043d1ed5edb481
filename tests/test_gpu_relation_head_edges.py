"""GPU (-m gpu): every C entry of the relation head (egtr_amd/csrc/rel_head.hip, rel_head_bf16.hip) at every slot count and at the
shape edges, BIT FOR BIT against the float64 restatement tests/relation_head_restated.py on the grid inputs, whose exactness
tests/test_relation_head_cases_cpu.py proves case by case (same seeds, same tensors).  The entries are called directly through
``_lib.launch`` with every output NaN-filled first, so a pair that a kernel never writes shows -- in the saved activations and the
dz workspace too.  "Bit for bit": of the float64 result cast to float32, a zero of either sign being a zero (``bits`` there).

Forward entries ("f32" = egtr_rel_head_forward_save_f32 with and without the save buffers, "x6", "x6_save", "bf16r_save", "bf16w",
"bf16p" fed with fp32 and with bf16 tables through egtr_rel_head_pack_tables_bf16):
  * T sweep at (2, 9, 33): every instantiation 1..10 (x6: 1..9; the two training entries: 4 and 7), i.e. every hand-counted wait of
    the table loads; the slot-sweep gates at T = 7, 9, 10 make each slot the ONLY open one of some pair (slots 8, 9: the second
    operand half of the packed tables);
  * N sweep at T = 7, R = 50, B = 3 with the frequency bias: N = 1 .. 65, ragged in both tile directions (8 x 4 pairs in the fp32 /
    x6 kernels, 4 x 8 in bf16p, 32 consecutive pairs in bf16w), ragged 2 x 4 super-blocks of bf16p at N = 65;
  * (5, 65, 7, 50): 135 super-blocks for at most 128 workgroups per MLP, some take a second trip of bf16p's persistent loop;
  * R sweep: both sides of the output-tile boundary 32 / 33 and of bf16p's W3-in-LDS boundary 60 / 61;
  * gate_mean of the same launches against the exact count of 0 / 0.5 / 1 gates;
  * containment of a non-finite table entry in its row / column of its image (bf16p: in its tile group, pinned), the refusals.
Backward (egtr_rel_head_backward_pairs_f32): every T, the four-wave split of the running index, both sides of the 256 chunk,
bitwise with the dz workspace; real-valued inputs against float64 under a derived worst-case rounding bound.

What the grid does NOT see: the accuracy of expf / __expf (its arguments are 0 and +-200 or more), the split pieces below the
leading one (every operand is a bf16 number: the middle and low pieces are zero), and the rounding of real-valued gates, tables
and activations to bf16.  The real-valued backward and containment tests below and the random-input tests of test_gpu_kernels.py,
test_gpu_token_x6.py and test_gpu_rel_head_matmul_precision.py cover those.  Nothing here looks at the generated code."""
import functools
import math

import pytest
import torch

import relation_head_restated as RH
from test_relation_head_cases_cpu import KEYS, bits, real_backward_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
FORWARD = ("f32", "f32_nosave", "x6", "x6_save", "bf16r_save", "bf16w", "bf16p", "bf16p_bf16tab")


def _entries(T):
    """the forward entries that serve T slots"""
    return [e for e in FORWARD if not (e == "x6" and T > 9) and not (e in ("x6_save", "bf16r_save") and T not in (4, 7))]


def _launch(entry, d, declare=None, node_cls="given", into=None):
    """One forward entry on the tensors of ``d`` (device, float32; bf16 operands are made here).  Returns dict(rel, conn, gm, h1,
    h2) -- h1 / h2 None where the entry has no save buffers.  ``declare``: integers to pass instead of the tensors' own T / R /
    hidden, ``into``: a dict that receives the output tensors before anything is launched (the refusal tests)."""
    from egtr_amd import _lib, ops
    B, N, T = d["gate_q"].shape
    R = d["w3r"].shape[0]
    P = B * N * N
    n = dict(T=T, R=R, hidden=256)
    n.update(declare or {})
    out = dict(rel=torch.full((B, N, N, R), NAN, device=DEV), conn=torch.full((B, N, N), NAN, device=DEV),
               gm=torch.zeros(T, device=DEV), h1=None, h2=None)
    save = entry in ("f32", "x6_save", "bf16r_save")
    if save:
        out["h1"], out["h2"] = torch.full((2, P, 256), NAN, device=DEV), torch.full((2, P, 256), NAN, device=DEV)
    if into is not None:
        into.update(out)
    trip = d.get("triplet")
    ncls = d.get("node_cls") if node_cls == "given" else None
    tail = [_lib.ptr(trip), _lib.ptr(ncls), B, N, n["T"], n["hidden"], n["R"], 0 if trip is None else trip.shape[0],
            out["rel"].data_ptr(), out["conn"].data_ptr(), out["gm"].data_ptr()]
    keep = []   # operands made here stay referenced until the launch is queued

    def p(*names):
        return [d[k].data_ptr() for k in names]

    def bf(k):
        keep.append(d[k].bfloat16().contiguous())
        return keep[-1].data_ptr()

    if entry in ("f32", "f32_nosave"):
        _lib.launch("egtr_rel_head_forward_save_f32", *p(*RH.NAMES), *tail, _lib.ptr(out["h1"]), _lib.ptr(out["h2"]))
    elif entry in ("x6", "x6_save", "bf16r_save"):
        w2xr, w3x, w2xc = ops.rel_head_streams(d["w2r"], d["w3r"][:64], d["w2c"], terms=1 if entry == "bf16r_save" else 6)
        keep += [w2xr, w3x, w2xc]
        args = p("gate_q", "gate_k", "uq", "uk", "b1") + [w2xr.data_ptr()] + p("b2r") + [w3x.data_ptr()] + p("b3r") + \
            [w2xc.data_ptr()] + p("b2c", "w3c", "b3c") + tail
        if entry == "x6":
            _lib.launch("egtr_rel_head_forward_bf16x6_f32", *args, 0)
        else:
            _lib.launch("egtr_rel_head_forward_" + ("bf16x6" if entry == "x6_save" else "bf16r") + "_save_f32", *args,
                        out["h1"].data_ptr(), out["h2"].data_ptr())
    else:
        mid = [d["b1"].data_ptr(), bf("w2r"), d["b2r"].data_ptr(), bf("w3r"), d["b3r"].data_ptr(), bf("w2c"), d["b2c"].data_ptr(),
               bf("w3c"), d["b3c"].data_ptr()]
        if entry == "bf16w":
            _lib.launch("egtr_rel_head_forward_bf16w", *p("gate_q", "gate_k", "uq", "uk"), *mid, *tail)
        else:
            pk = []
            for k in ("uq", "uk"):
                t = d[k].bfloat16().contiguous() if entry == "bf16p_bf16tab" else d[k]
                pk.append(torch.full((B * N, 8192), NAN, dtype=torch.bfloat16, device=DEV))
                keep.append(t)
                _lib.launch("egtr_rel_head_pack_tables_bf16", t.data_ptr(), int(t.dtype == torch.bfloat16), B * N, T,
                            pk[-1].data_ptr())
            _lib.launch("egtr_rel_head_forward_bf16p", *p("gate_q", "gate_k"), pk[0].data_ptr(), pk[1].data_ptr(), *mid, *tail)
    torch.cuda.synchronize()
    return out


def _where(entry, B, N, b, i, j):
    """the tile and lane of pair (b, i, j) in the entry's kernel"""
    if entry.startswith("bf16p"):
        it, jt = i // 4, j // 8
        return (f"bf16p tile (it {it}, jt {jt}) = wave {(it & 1) * 4 + (jt & 3)} of super-block ({it >> 1}, {jt >> 2}), "
                f"lanes {(i % 4) * 8 + j % 8} and +32")
    if entry == "bf16w":
        p = (b * N + i) * N + j
        return f"wave {p // 32} (32 consecutive pairs), lanes {p % 32} and +32"
    return f"8 x 4 tile (i0 {i // 8 * 8}, j0 {j // 4 * 4}), lanes {(i % 8) * 4 + j % 4} and +32"


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
                b, i, j, tag = idx[0], idx[1], idx[2], (f"relation {idx[3]}" if name == "rel" else "connectivity")
            raise AssertionError(f"{what}{entry}: {name} differs in {int(ne.sum())} of {ne.numel()} elements, first at (b {b}, i {i}, "
                                 f"j {j}), {tag}: got {float(a[tuple(idx)])!r}, want {float(want[tuple(idx)])!r}; "
                                 + _where(entry, B, N, b, i, j))


def _gate_mean_adds(entry, B, N):
    """fp32 atomic adds of ``v / total`` into each gate_mean[t]: wave 0 of every 8 x 4 tile in the two-wave kernels (fp32, x6), the
    one wave of every 32 consecutive pairs in bf16w, the one wave of every 4 x 8 tile in bf16p"""
    if entry.startswith("bf16p"):
        return B * ((N + 3) // 4) * ((N + 7) // 8)
    if entry == "bf16w":
        return (B * N * N + 31) // 32
    return B * ((N + 7) // 8) * ((N + 3) // 4)


def _check_gate_mean(entry, gm, want, B, N):
    """``want``: the exact count of 0 / 0.5 / 1 gates over B N N, float64.  Each add rounds once and each addend carries the
    rounding of its quotient: (adds + 2) ulps of the result bound what the sum can lose."""
    adds = _gate_mean_adds(entry, B, N)
    for t, (g, w) in enumerate(zip(gm.cpu().double().tolist(), want.tolist())):
        bound = (adds + 2) * 2.0 ** (math.floor(math.log2(w)) - 23) if w > 0 else 0.0
        assert abs(g - w) <= bound, f"{entry}: gate_mean[{t}] = {g!r}, exact {w!r}, |diff| {abs(g - w):.3e} > {bound:.3e} ({adds} adds)"


@functools.lru_cache(maxsize=4)
def _case(case):
    """(inputs on the device, float64 reference cast to float32 on the device, exact gate means); never written to"""
    B, N, T, R, C1, sweep = case
    d = RH.grid_inputs(RH.case_seed(*case), B, N, T, R, C1, sweep)
    gm = RH.gate_mean_exact(d["gate_q"], d["gate_k"])
    d = {k: v.to(DEV) for k, v in d.items()}
    rel, conn, _, h1, h2 = RH.forward(d)
    assert rel.dtype == torch.float64
    return d, dict(rel=rel.float(), conn=conn.float(), h1=h1.float(), h2=h2.float()), gm


def _run_case(case, entries):
    B, N, T = case[:3]
    d, ref, gm = _case(case)
    for entry in entries:
        out = _launch(entry, d)
        _check_bits(entry, out, ref, RH.case_id(case) + " ")
        _check_gate_mean(entry, out["gm"], gm, B, N)


# ---- 1. forward, grid inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RH.T_SWEEP, ids=RH.case_id)
def test_forward_every_slot_count_is_bitwise_the_float64_restatement(case):
    """(2, 9, T, 33) for T = 1 .. 10 and the slot-sweep gates at T = 7, 9, 10: N = 9 is ragged for 8 x 4 and 4 x 8 tiles, R = 33
    takes the second output tile.  Before this test T = 2, 3, 5, 6, 8 ran nowhere and T = 10 only in the bf16 forward."""
    _run_case(case, _entries(case[2]))


def test_forward_sweeps_launch_every_instantiation():
    """the T sweep above reaches each (entry, T) the C entries dispatch on"""
    ran = {(e, c[2]) for c in RH.T_SWEEP for e in _entries(c[2])}
    for e in FORWARD:
        want = range(1, 10) if e == "x6" else (4, 7) if e in ("x6_save", "bf16r_save") else range(1, 11)
        assert {T for (x, T) in ran if x == e} == set(want), e


@pytest.mark.parametrize("case", RH.N_SWEEP, ids=RH.case_id)
def test_forward_every_query_count_edge_is_bitwise_the_float64_restatement(case):
    """T = 7, R = 50, B = 3, frequency bias on with classes 0 and C1 - 1: N = 1, N < 4, whole and ragged tiles of every kernel"""
    _run_case(case, _entries(7))


@pytest.mark.parametrize("case", RH.PERSISTENT, ids=RH.case_id)
def test_bf16p_second_trip_of_the_persistent_loop_is_bitwise(case):
    """5 images x 9 x 3 super-blocks = 135 > 128 workgroups per MLP (256 CUs, one workgroup per CU, even ids the relation MLP)"""
    B, N = case[:2]
    it_n, jt_n = (N + 3) // 4, (N + 7) // 8
    assert B * ((it_n + 1) // 2) * ((jt_n + 3) // 4) == 135
    assert torch.cuda.get_device_properties(0).multi_processor_count // 2 < 135
    _run_case(case, ["bf16p", "bf16p_bf16tab"])


@pytest.mark.parametrize("case", RH.R_SWEEP, ids=RH.case_id)
def test_forward_every_relation_count_edge_is_bitwise_the_float64_restatement(case):
    """(2, 9, 7, R): R = 1, 31 | 32 | 33 (second output tile), 60 | 61 (W3 of bf16p in LDS or not), 64; without and with the
    frequency bias"""
    _run_case(case, _entries(7))


# ---- 2. backward --------------------------------------------------------------------------------------------------------------------
def _backward(dh1, gate_q, gate_k, uq, uk, declare=None):
    from egtr_amd import _lib
    B, N, T = gate_q.shape
    n = dict(T=T, hidden=256)
    n.update(declare or {})
    out = dict(duq=torch.full_like(uq, NAN), duk=torch.full_like(uk, NAN), dgate_q=torch.full_like(gate_q, NAN),
               dgate_k=torch.full_like(gate_k, NAN), dz=torch.full((B, N, N, T), NAN, device=DEV))
    _lib.launch("egtr_rel_head_backward_pairs_f32", dh1.data_ptr(), gate_q.data_ptr(), gate_k.data_ptr(), uq.data_ptr(),
                uk.data_ptr(), B, N, n["T"], n["hidden"], out["duq"].data_ptr(), out["duk"].data_ptr(), out["dgate_q"].data_ptr(),
                out["dgate_k"].data_ptr(), out["dz"].data_ptr())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", RH.BACKWARD_CASES, ids=RH.case_id)
def test_backward_pairs_grid_is_bitwise_the_float64_restatement(case):
    """every T at (2, 9) -- T = 2, 3, 5, 6, 8 and 10 (90 KiB of static LDS) for the first time --, N around the four-wave split of
    the running index at T = 7, N = 255 | 256 | 257 around the 256 chunk at T = 2 and 10.  One dropped pair changes an integer."""
    B, N, T = case
    d = RH.grid_inputs(RH.case_seed(*case), B, N, T, 1)
    a = [x.to(DEV) for x in (RH.grid_dh1(RH.case_seed(*case) + 1, B, N), d["gate_q"], d["gate_k"], d["uq"], d["uk"])]
    ref = RH.backward_pairs(*a, want_mag=False)[0]
    out = _backward(*a)
    for k in KEYS:
        want = ref[k].float()
        ne = bits(out[k]) != bits(want)
        if bool(ne.any()):
            idx = tuple(int(x) for x in ne.nonzero()[0])
            raise AssertionError(f"{RH.case_id(case)}: {k} differs in {int(ne.sum())} of {ne.numel()} elements, first at "
                                 f"(b, row, ...) = {idx}: got {float(out[k][idx])!r}, want {float(want[idx])!r}")


@pytest.mark.parametrize("case", RH.BACKWARD_REAL, ids=RH.case_id)
def test_backward_pairs_real_valued_within_the_derived_rounding_bound(case):
    """Standard-normal gates, tables and dh1; |got - ref| <= (n + 8) 2^-24 mag per element (``RH.backward_bound``).  dh1 is an
    INPUT here, so no ReLU can flip between fp32 and float64: a worst-case rounding bound is usable.
    Largest |err| / bound measured on the MI355X: 0.062 (dz at (1, 257, 4)); duq / duk 0.048 at (2, 40, 7) and 0.007 at (1, 257, 4),
    the gate gradients below 0.001.  torch's own fp32 evaluation of the formulas stays below 0.25 (the CPU file asserts that)."""
    B, N, T = case
    a = [x.to(DEV) for x in real_backward_inputs(B, N, T)]
    ref, mag = RH.backward_pairs(*a)
    bound = RH.backward_bound(mag, N)
    out = _backward(*a)
    worst = {}
    for k in KEYS:
        assert bool(torch.isfinite(out[k]).all()), k
        worst[k] = float(((out[k].double() - ref[k]).abs() / bound[k]).max())
        print(f"backward {RH.case_id(case)} {k}: max |err| / bound = {worst[k]:.4f}")
    assert max(worst.values()) <= 1.0, worst


# ---- 3. containment of non-finite table entries -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _real():
    d = RH.random_inputs(4242, 2, 13, 7, 50)
    return {k: v.to(DEV) for k, v in d.items()}


def _footprint(entry, table, q, N):
    """the subject rows (uq) / object columns (uk) of its image that a non-finite table entry of query q reaches: q alone, except
    in bf16p the 4 subjects / 8 objects that share a tile with q"""
    if not entry.startswith("bf16p"):
        return [q]
    group = 4 if table == "uq" else 8
    return list(range(q // group * group, min(q // group * group + group, N)))


@pytest.mark.parametrize("entry", FORWARD)
@pytest.mark.parametrize("table,at,value", [("uq", (1, 5, 2), NAN), ("uk", (0, 9, 6), float("inf"))], ids=["nan_uq", "inf_uk"])
def test_a_non_finite_table_entry_stays_in_its_row_or_column(entry, table, at, value):
    """(2, 13, 7, 50), random real-valued inputs.  One channel of uq[1, 5, 2] = NaN / of uk[0, 9, 6] = +inf, once in the relation
    half and once in the connectivity half: every pair of subject row 5 of image 1 (object column 9 of image 0) is non-finite in
    the output of that MLP, and every other element of both outputs keeps the bits of the clean launch -- the reference's
    footprint (relu(NaN) = NaN is kept on purpose, common.h).
    bf16p deviates, and its footprint is pinned EXACTLY (``_footprint``; DESIGN.md, "relation head"): its layer 1 is a matrix
    product over the 12 row sets of a 4 x 8 tile whose gate operand is zero for the pairs that do not use a row set, and
    0 x NaN = NaN, so the entry reaches the whole 4-subject group of row 5 (rows 4-7) or 8-object group of column 9 (columns 8-12)
    of that image -- all of it, and nothing outside it.  Two fixes (flagging the row while packing, NaN written by the forward)
    were correct on this test and measured 4 % slower on the stress shape, outside the run-to-run spread; neither was kept."""
    d = _real()
    clean = _launch(entry, d)
    assert bool(torch.isfinite(clean["rel"]).all()) and bool(torch.isfinite(clean["conn"]).all())
    b, q, t = at
    for half, (hit, other) in enumerate((("rel", "conn"), ("conn", "rel"))):
        x = dict(d)
        x[table] = d[table].clone()
        x[table][b, q, t, 256 * half + 77] = value
        out = _launch(entry, x)
        mask = torch.zeros(2, 13, 13, dtype=torch.bool, device=DEV)
        reach = _footprint(entry, table, q, 13)
        if table == "uq":
            mask[b, reach, :] = True
        else:
            mask[b, :, reach] = True
        got = out[hit].reshape(2, 13, 13, -1)
        fin = torch.isfinite(got)
        assert not bool(fin[mask].any()), f"{entry}: finite {hit} output inside the footprint {reach}"
        same = (bits(got) == bits(clean[hit].reshape(2, 13, 13, -1))).all(-1)
        spilled = (~same & ~mask).nonzero().tolist()
        assert not spilled, (f"{entry}: {hit} changed outside the footprint {reach} at (b, i, j) = "
                             f"{spilled[:12]} ({len(spilled)} pairs)")
        assert torch.equal(bits(out[other]), bits(clean[other])), f"{entry}: {other} changed by a {hit}-half channel"


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def _untouched(out):
    return all(bool(torch.isnan(out[k]).all()) for k in ("rel", "conn", "h1", "h2") if out[k] is not None) and \
        bool((out["gm"] == 0).all())


@pytest.mark.parametrize("entry", FORWARD)
def test_forward_entries_refuse_what_they_do_not_serve(entry):
    """num_rel = 65, a slot count past the entry's range, hidden = 128: the binding's error (status -3), nothing written.  The
    operands have the declared sizes, so a check that let one through would still stay inside its buffers."""
    from egtr_amd import _lib
    bad_T = [10] if entry == "x6" else [1, 5, 10] if entry in ("x6_save", "bf16r_save") else [11]
    for T, R, declare in [(7, 65, None)] + [(T, 50, None) for T in bad_T] + [(7, 50, dict(hidden=128))]:
        d = {k: v.to(DEV) for k, v in RH.random_inputs(5, 1, 5, T, R).items()}
        out = {}
        with pytest.raises(_lib.EgtrHipError, match=r"status -3"):
            _launch(entry, d, declare=declare, into=out)
        torch.cuda.synchronize()
        assert _untouched(out), (entry, T, R, declare)


def test_backward_entry_refuses_what_it_does_not_serve():
    from egtr_amd import _lib
    for T, declare in ((11, None), (7, dict(hidden=128))):
        d = RH.random_inputs(6, 1, 5, T, 1)
        a = [x.to(DEV) for x in (torch.randn(2, 25, 256), d["gate_q"], d["gate_k"], d["uq"], d["uk"])]
        B, N = 1, 5
        bufs = [torch.full_like(a[3], NAN), torch.full_like(a[4], NAN), torch.full_like(a[1], NAN), torch.full_like(a[2], NAN),
                torch.full((B, N, N, T), NAN, device=DEV)]
        n = dict(T=T, hidden=256)
        n.update(declare or {})
        with pytest.raises(_lib.EgtrHipError, match=r"status -3"):
            _lib.launch("egtr_rel_head_backward_pairs_f32", *[x.data_ptr() for x in a], B, N, n["T"], n["hidden"],
                        *[x.data_ptr() for x in bufs])
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(x).all()) for x in bufs)


@pytest.mark.parametrize("entry", FORWARD)
def test_frequency_bias_without_node_classes_is_an_argument_error(entry):
    from egtr_amd import _lib
    d = {k: v.to(DEV) for k, v in RH.random_inputs(7, 1, 5, 7, 50, 6).items()}
    with pytest.raises(_lib.EgtrHipError, match=r"status -1"):
        _launch(entry, d, node_cls=None)
