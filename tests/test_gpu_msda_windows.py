"""GPU (-m gpu): the MSDA backward at the edges of the value-tile kernel's window bookkeeping (csrc/msda_tile.hip) -- chunk and
column-tile seams, empty windows, degenerate levels, L = 1 with P = 16, gapped levels, more than 65 536 window pixels -- through
every route, element by element against the float64 restatement and its error budgets (tests/msda_restated.py; the
criteria are those of ``check_backward`` / ``check_forward`` there, derived from the count of fp32 roundings, not tuned).
tests/test_msda_cases_cpu.py proves on the CPU that each case has the windows it is named for.

Routes of a case: the explicit variants 1 (wave per query, per-sample atomics), 2 (wave per query + value tiles) and
3 (generic), the automatic entry, the deterministic entry (twice, bit-equal), bfloat16 operands on the default and the
deterministic entry of the module (bfloat16 grad_value) and of the C ABI (fp32 grad_value).  Each test prints its worst error-to-bound ratios.
"""
import functools

import pytest
import torch

import hip_test_abi as TA
import msda_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPERANDS = ("value", "shapes", "lsi", "loc", "attn", "grad_out")


def _kernels():
    from egtr_amd.load_custom import load_hip_kernels
    return load_hip_kernels()


def _pyramid(x):
    return [tuple(s) for s in x["shapes"].tolist()]


def case(name, bf16=False):
    return _case(name, bool(bf16))


@functools.lru_cache(maxsize=None)
def _case(name, bf16):
    """(host operands, device operands, float64 reference with budgets): built once, left unchanged.  bf16: value and
    grad_out rounded to bfloat16, the reference computed from the rounded values.  The cases beyond 65 536 pixels run the
    restatement on their `rows` only -- every other query has grad_out = 0 and contributes exactly nothing."""
    if bf16:
        x = dict(case(name)[0])
        x["value"], x["grad_out"] = x["value"].to(torch.bfloat16), x["grad_out"].to(torch.bfloat16)
    else:
        x = (R.CASES.get(name) or R.BIG_CASES.get(name) or R.BOUNDARY_CASE)()
    rows = x.get("rows")
    sub = (lambda t: t) if rows is None else (lambda t: t[:, rows])
    ref = R.msda_backward_budget(x["value"].float(), _pyramid(x), x["lsi"].tolist(), sub(x["loc"]), sub(x["attn"]),
                                 sub(x["grad_out"].float()))
    return x, {n: x[n].to(DEV) for n in OPERANDS}, ref


def auto_entry(d, deterministic=False):
    from egtr_amd import ops
    with ops.deterministic(deterministic):
        out = _kernels().ms_deform_attn_backward(d["value"], d["shapes"], d["lsi"], d["loc"], d["attn"], d["grad_out"], 64)
    torch.cuda.synchronize()
    return out


def explicit(d, variant):
    out = TA.msda_backward_variant(d["value"], d["shapes"], d["lsi"], d["loc"], d["attn"], d["grad_out"], variant)
    torch.cuda.synchronize()
    return out


def c_entries_bf16(d, label, ref, rows):
    """egtr_msda_backward_bf16 / _det_bf16 themselves: bf16 operands, grad_value still fp32 -- the fp32 criteria apply in full
    (behind the module's rounding of grad_value to bfloat16 a small lost contribution could hide)."""
    from egtr_amd import _lib, ops
    lib = _lib.lib()
    B, S, Mh, Dc = d["value"].shape
    Lq, L, P = d["loc"].shape[1], d["shapes"].shape[0], d["loc"].shape[4]
    assert int(lib.egtr_msda_backward_bf16_workspace_floats(B, S, Mh, Dc, L, Lq, P)) == 0
    ws = torch.empty(int(lib.egtr_msda_backward_det_workspace_bytes(B, S, Mh, Dc)), dtype=torch.uint8, device=DEV)
    for entry, what in ((lib.egtr_msda_backward_bf16, None), (lib.egtr_msda_backward_det_bf16, ws.data_ptr())):
        gv = torch.zeros(d["value"].shape, dtype=torch.float32, device=DEV)
        gl, ga = torch.empty_like(d["loc"]), torch.empty_like(d["attn"])
        _lib.check(entry(ops._stream(), d["grad_out"].data_ptr(), d["value"].data_ptr(), d["shapes"].data_ptr(),
                         d["lsi"].data_ptr(), d["loc"].data_ptr(), d["attn"].data_ptr(), B, S, Mh, Dc, L, Lq, P,
                         gv.data_ptr(), gl.data_ptr(), ga.data_ptr(), what), "msda backward bf16")
        torch.cuda.synchronize()
        ratios = R.check_backward(f"{label} {'det' if what else 'default'} entry", (gv, gl, ga), ref, rows=rows)
    return ratios


def run_route(name, route):
    bf16 = route.endswith("bf16")
    x, d, ref = case(name, bf16)
    label = f"{name} [{route}]"
    if route == "c_entries_bf16":
        return c_entries_bf16(d, label, ref, x.get("rows"))
    if route.startswith("variant"):
        got = explicit(d, int(route[-1]))
    elif route.startswith("deterministic"):
        got = auto_entry(d, True)
        again = auto_entry(d, True)
        for a, b, what in zip(got, again, ("grad_value", "grad_loc", "grad_attn")):
            assert torch.equal(a, b), (label, what, "two deterministic runs differ")
    else:
        got = auto_entry(d)
    assert got[0].dtype == x["value"].dtype and got[1].dtype == got[2].dtype == torch.float32
    return R.check_backward(label, got, ref, bf16=bf16, rows=x.get("rows"))


ROUTES = ["variant1", "variant2", "variant3", "auto", "deterministic", "auto_bf16", "deterministic_bf16", "c_entries_bf16"]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", list(R.CASES))
def test_window_case(name, route):
    """seams: S = Lq = 2720, B = 3, 43 tiles per image = 129 items per head on 32 workgroups; selected items have windows of
    1, 31, 32, 33, 447, 448, 449, 895, 896, 897 and 2720 columns made of two or more levels, and on heads 0, 1, 2 and 7 the
    second item of a workgroup is smaller than its first (msda_restated.SEAM_FIRST / SEAM_SECOND).
    empty: a tile whose level 0 is empty for every head, and two items without any sample in range (ntot = 0) followed by
    ordinary ones on their workgroups.  degenerate: levels (17, 16), (1, 9), (9, 1), (1, 1).  l1_*: L = 1, P = 16 through the
    tile pair (Lq = S = 256), four waves per query (Lq = 40) and one wave per query with atomics (Lq = 5000).  gapped:
    level_start_index [0, 261] with S = Lq = 325 -- consecutive-query tiles."""
    run_route(name, route)


def test_gap_rows_stay_zero():
    x, d, ref = case("gapped")
    assert float(ref["abs_grad_value"][:, 256:261].max()) == 0
    for got in (explicit(d, 1), explicit(d, 2), explicit(d, 3), auto_entry(d), auto_entry(d, True)):
        assert float(got[0][:, 256:261].abs().max()) == 0


@pytest.mark.parametrize("variant", [1, 3])
@pytest.mark.parametrize("name", ["l1_tile", "l1_split4", "l1_split1"])
def test_forward_one_level_sixteen_points(name, variant):
    x, d, _ = case(name)
    ref = R.msda_forward_budget(x["value"], _pyramid(x), x["lsi"].tolist(), x["loc"], x["attn"])
    out = TA.msda_forward_variant(d["value"], d["shapes"], d["lsi"], d["loc"], d["attn"], variant)
    torch.cuda.synchronize()
    R.check_forward(f"{name} forward [variant{variant}]", out, ref)


@pytest.mark.parametrize("route", ["auto", "deterministic", "auto_bf16", "c_entries_bf16", "variant1"])
@pytest.mark.parametrize("name", list(R.BIG_CASES))
def test_beyond_sixteen_bit_windows(name, route):
    """S = Lq = 65 792 (one level of 257 x 256) and 66 852 (four levels, none above 65 536 alone), B = 1: the items of three
    tiles have windows of S columns for every head.  The value-tile kernel keeps a window pixel id in 16 bits, so such calls
    go to the per-sample route (variant 1), which also has to clear grad_value (the deterministic accumulators) itself:
    the full grad_value, and grad_loc / grad_attn of the rows with a nonzero grad_out, meet the criteria."""
    run_route(name, route)


@pytest.mark.parametrize("name", list(R.BIG_CASES))
def test_explicit_value_tiles_beyond_sixteen_bits_are_refused(name):
    from egtr_amd._lib import EgtrHipError
    _, d, _ = case(name)
    with pytest.raises(EgtrHipError, match="status -3"):
        explicit(d, 2)


def test_sixty_five_thousand_five_hundred_thirty_six_pixels_are_served_by_value_tiles():
    """S = Lq = 65 536 (one level of 256 x 256): the windows of the case's three tiles are all of S, so ids reach 65 535, the
    last that fit into 16 bits.  Explicit variant 2 and the automatic entry (which takes it) against variant 1."""
    x, d, ref = case("boundary")
    assert x["value"].shape[1] == 65536
    for variant in (2, 1):
        R.check_backward(f"boundary [variant{variant}]", explicit(d, variant), ref, rows=x["rows"])
    R.check_backward("boundary [auto]", auto_entry(d), ref, rows=x["rows"])
    run_route("boundary", "deterministic")


@pytest.mark.parametrize("name", list(R.BIG_CASES))
def test_entries_beyond_sixteen_bits_clear_what_they_accumulate_into(name):
    """egtr_msda_backward_out_f32 with grad_value full of NaN, egtr_msda_backward_det_f32 with NaN in grad_value and every
    workspace byte set: encoder-shaped calls above 65 536 pixels do not run the kernel pair that clears rows in passing."""
    from egtr_amd import _lib, ops
    lib = _lib.lib()
    x, d, ref = case(name)
    B, S, Mh, Dc = d["value"].shape
    Lq, L, P = d["loc"].shape[1], d["shapes"].shape[0], d["loc"].shape[4]
    ws = torch.full((int(lib.egtr_msda_backward_det_workspace_bytes(B, S, Mh, Dc)),), 0xFF, dtype=torch.uint8, device=DEV)
    for entry, extra in ((lib.egtr_msda_backward_out_f32, ()), (lib.egtr_msda_backward_det_f32, (ws.data_ptr(),))):
        gv = torch.full_like(d["value"], float("nan"))
        gl = torch.full_like(d["loc"], float("nan"))
        ga = torch.full_like(d["attn"], float("nan"))
        _lib.check(entry(ops._stream(), d["grad_out"].data_ptr(), d["value"].data_ptr(), d["shapes"].data_ptr(),
                         d["lsi"].data_ptr(), d["loc"].data_ptr(), d["attn"].data_ptr(), B, S, Mh, Dc, L, Lq, P,
                         gv.data_ptr(), gl.data_ptr(), ga.data_ptr(), *extra), "msda backward")
        torch.cuda.synchronize()
        R.check_backward(f"{name} [{'det' if extra else 'out'} entry, NaN-filled]", (gv, gl, ga), ref, rows=x["rows"])
